// AmpliSolveNormalExceedance -- how many normals of the panel show an allele at a tumour's fraction or above, and the cells that top
// (nearly) all of them on both strands, in the reference's key=value style.
//   AmpliSolveNormalExceedance panel_design=<bed> reference_genome=<fa> germline_dir=<dir> tumour_dir=<dir|-> output_dir=<dir>
//                              coverage_cutoff=<i> calling_cutoff=<i> min_alt_reads=<i> min_vaf_pm=<i> min_normals=<i> max_normals=<i>
// Exactly 11 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::ExArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveNormalExceedance panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir or -> "
                            "output_dir=<dir> coverage_cutoff=<int> calling_cutoff=<int> min_alt_reads=<int> min_vaf_pm=<int> min_normals=<int> max_normals=<int>\n"
                            "\tAll arguments are required, in this order (usual values: coverage_cutoff=100 calling_cutoff=100 min_alt_reads=3 min_vaf_pm=0 "
                            "min_normals=10 max_normals=0).";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design},     {"reference_genome", &A::reference_genome}, {"germline_dir", &A::germline_dir},
                                        {"tumour_dir", &A::tumour_dir},         {"output_dir", &A::output_dir},             {"coverage_cutoff", &A::coverage_cutoff},
                                        {"calling_cutoff", &A::calling_cutoff}, {"min_alt_reads", &A::min_alt_reads},       {"min_vaf_pm", &A::min_vaf_pm},
                                        {"min_normals", &A::min_normals},       {"max_normals", &A::max_normals}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_normal_exceedance, &A::refbases_file); }
