// AmpliSolvePanelDispersion -- per-position dispersion of a panel of normals and per-normal outlier scores, in the
// reference's key=value style.
//   AmpliSolvePanelDispersion panel_design=<bed> reference_genome=<fa> germline_dir=<dir> coverage_cutoff=<i> z_cutoff=<f> output_dir=<dir>
// Exactly 6 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 7) {
        std::cout << "Usage:\n\tAmpliSolvePanelDispersion panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> coverage_cutoff=<int> "
                     "z_cutoff=<float> output_dir=<dir>\n\tAll arguments are required, in this order." << std::endl;
        return 1;
    }
    ampli::PdArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.reference_genome = token(argv[2], "reference_genome");
    a.germline_dir = token(argv[3], "germline_dir");
    a.coverage_cutoff = token(argv[4], "coverage_cutoff");
    a.z_cutoff = token(argv[5], "z_cutoff");
    a.output_dir = token(argv[6], "output_dir");
    if (const char *e = getenv("AMPLISOLVE_REFBASES_FILE")) a.refbases_file = e;
    return ampli::finish(ampli::run_panel_dispersion(a));
}
