// AmpliSolveAmpliconCoverage -- amplicon coverage and copy ratio of the normals and the tumours of a panel against the panel of normals
// (DESIGN 16), in the reference's key=value style.
//   AmpliSolveAmpliconCoverage panel_design=<bed> germline_dir=<dir> tumour_dir=<dir|-> output_dir=<dir> coverage_cutoff=<i> min_normals=<i>
//                              min_amplicons=<i> z_cutoff=<f> gain_ratio=<f> loss_ratio=<f> exclude_chrom=<comma list|->
// Exactly 11 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::AcArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveAmpliconCoverage panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> output_dir=<dir> "
                            "coverage_cutoff=<int> min_normals=<int> min_amplicons=<int> z_cutoff=<float> gain_ratio=<float> loss_ratio=<float> "
                            "exclude_chrom=<comma list or ->\n\tAll arguments are required, in this order (usual values: coverage_cutoff=100 "
                            "min_normals=5 min_amplicons=3 z_cutoff=3 gain_ratio=1.3 loss_ratio=0.7 exclude_chrom=chrX,chrY).";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design},   {"germline_dir", &A::germline_dir},       {"tumour_dir", &A::tumour_dir},
                                        {"output_dir", &A::output_dir},       {"coverage_cutoff", &A::coverage_cutoff}, {"min_normals", &A::min_normals},
                                        {"min_amplicons", &A::min_amplicons}, {"z_cutoff", &A::z_cutoff},               {"gain_ratio", &A::gain_ratio},
                                        {"loss_ratio", &A::loss_ratio},       {"exclude_chrom", &A::exclude_chrom}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_amplicon_coverage); }
