// AmpliSolvePanelDispersion -- per-position dispersion of a panel of normals and per-normal outlier scores, in the
// reference's key=value style.
//   AmpliSolvePanelDispersion panel_design=<bed> reference_genome=<fa> germline_dir=<dir> coverage_cutoff=<i> z_cutoff=<f> output_dir=<dir>
// Exactly 6 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "host.hpp"

static std::string token(const char *arg, const char *key)
{
    char buf[4096];
    buf[0] = 0;
    std::string fmt = std::string(key) + "=%4000s";
    sscanf(arg, fmt.c_str(), buf);
    return buf;
}

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
    const int rc = ampli::run_panel_dispersion(a);
    std::cout.flush();
    ampli::finish_process(rc ? 1 : 0);
    return rc ? 1 : 0;
}
