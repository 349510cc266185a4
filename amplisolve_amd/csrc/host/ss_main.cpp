// AmpliSolveSubstitutionSpectrum -- per-file substitution spectrum and strand asymmetry of the normals and the tumours of a panel against
// the panel of normals, in the reference's key=value style.
//   AmpliSolveSubstitutionSpectrum panel_design=<bed> reference_genome=<fa> germline_dir=<dir> tumour_dir=<dir|-> output_dir=<dir>
//                                  coverage_cutoff=<i> max_alt_pm=<i> min_sites=<i> min_normals=<i> excess_ratio=<f> z_cutoff=<f> asym_delta=<f>
// Exactly 12 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 13) {
        std::cout << "Usage:\n\tAmpliSolveSubstitutionSpectrum panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir or -> "
                     "output_dir=<dir> coverage_cutoff=<int> max_alt_pm=<int> min_sites=<int> min_normals=<int> excess_ratio=<float> z_cutoff=<float> "
                     "asym_delta=<float>\n\tAll arguments are required, in this order (usual values: coverage_cutoff=100 max_alt_pm=30 min_sites=200 "
                     "min_normals=5 excess_ratio=3 z_cutoff=10 asym_delta=0.15)." << std::endl;
        return 1;
    }
    ampli::SsArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.reference_genome = token(argv[2], "reference_genome");
    a.germline_dir = token(argv[3], "germline_dir");
    a.tumour_dir = token(argv[4], "tumour_dir");
    a.output_dir = token(argv[5], "output_dir");
    a.coverage_cutoff = token(argv[6], "coverage_cutoff");
    a.max_alt_pm = token(argv[7], "max_alt_pm");
    a.min_sites = token(argv[8], "min_sites");
    a.min_normals = token(argv[9], "min_normals");
    a.excess_ratio = token(argv[10], "excess_ratio");
    a.z_cutoff = token(argv[11], "z_cutoff");
    a.asym_delta = token(argv[12], "asym_delta");
    if (const char *e = getenv("AMPLISOLVE_REFBASES_FILE")) a.refbases_file = e; // pre-computed chrom/pos/base table instead of the FASTA
    return ampli::finish(ampli::run_substitution_spectrum(a));
}
