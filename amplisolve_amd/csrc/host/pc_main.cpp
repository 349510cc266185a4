// AmpliSolvePairedComparison -- two count files of one patient tested against each other at every cell: tumour against matched normal,
// baseline against follow-up, replicate against replicate, in the reference's key=value style.
//   AmpliSolvePairedComparison panel_design=<bed> reference_genome=<fa> sample_dir=<dir> pairs=<file> depth_cutoff=<i> q_min=<f>
//                              min_vaf=<f> output_dir=<dir>
// Exactly 8 tokens in this order.  pairs: nameA<TAB>nameB per line, the names as the Summary names samples.  Not a drop-in: the exit
// status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::PcArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolvePairedComparison panel_design=<bed> reference_genome=<fasta> sample_dir=<dir> pairs=<file> depth_cutoff=<int> "
                            "q_min=<float> min_vaf=<float> output_dir=<dir>\n"
                            "\tAll arguments are required, in this order (usual values: depth_cutoff=100 q_min=13 min_vaf=0.005; pairs lists nameA<TAB>nameB per "
                            "line).";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design}, {"reference_genome", &A::reference_genome}, {"sample_dir", &A::sample_dir},
                                        {"pairs", &A::pairs},               {"depth_cutoff", &A::depth_cutoff},         {"q_min", &A::q_min},
                                        {"min_vaf", &A::min_vaf},           {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_paired_comparison, &A::refbases_file); }
