// AmpliSolveAmpliconCoverage -- amplicon coverage and copy ratio of the normals and the tumours of a panel against the panel of normals
// (DESIGN 16), in the reference's key=value style.
//   AmpliSolveAmpliconCoverage panel_design=<bed> germline_dir=<dir> tumour_dir=<dir|-> output_dir=<dir> coverage_cutoff=<i> min_normals=<i>
//                              min_amplicons=<i> z_cutoff=<f> gain_ratio=<f> loss_ratio=<f> exclude_chrom=<comma list|->
// Exactly 11 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 12) {
        std::cout << "Usage:\n\tAmpliSolveAmpliconCoverage panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> output_dir=<dir> "
                     "coverage_cutoff=<int> min_normals=<int> min_amplicons=<int> z_cutoff=<float> gain_ratio=<float> loss_ratio=<float> "
                     "exclude_chrom=<comma list or ->\n\tAll arguments are required, in this order (usual values: coverage_cutoff=100 "
                     "min_normals=5 min_amplicons=3 z_cutoff=3 gain_ratio=1.3 loss_ratio=0.7 exclude_chrom=chrX,chrY)." << std::endl;
        return 1;
    }
    ampli::AcArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.germline_dir = token(argv[2], "germline_dir");
    a.tumour_dir = token(argv[3], "tumour_dir");
    a.output_dir = token(argv[4], "output_dir");
    a.coverage_cutoff = token(argv[5], "coverage_cutoff");
    a.min_normals = token(argv[6], "min_normals");
    a.min_amplicons = token(argv[7], "min_amplicons");
    a.z_cutoff = token(argv[8], "z_cutoff");
    a.gain_ratio = token(argv[9], "gain_ratio");
    a.loss_ratio = token(argv[10], "loss_ratio");
    a.exclude_chrom = token(argv[11], "exclude_chrom");
    return ampli::finish(ampli::run_amplicon_coverage(a));
}
