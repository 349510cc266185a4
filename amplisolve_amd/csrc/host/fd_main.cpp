// AmpliSolveFalseDiscovery -- every tumour cell scored against the panel's error table, the Benjamini-Hochberg adjusted score of every
// cell per file, and the cells that pass at a false-discovery rate, in the reference's key=value style.
//   AmpliSolveFalseDiscovery panel_design=<bed> reference_genome=<fa> germline_dir=<dir> tumour_dir=<dir> C_value=<f>
//                            coverage_cutoff=<i> calling_cutoff=<i> fdr=<f> q_min=<f> output_dir=<dir>
// Exactly 10 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::FdArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveFalseDiscovery panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir> "
                            "C_value=<float> coverage_cutoff=<int> calling_cutoff=<int> fdr=<float> q_min=<float> output_dir=<dir>\n"
                            "\tAll arguments are required, in this order (usual values: C_value=0.002 coverage_cutoff=100 calling_cutoff=100 fdr=0.05 "
                            "q_min=13).";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design}, {"reference_genome", &A::reference_genome}, {"germline_dir", &A::germline_dir},
                                        {"tumour_dir", &A::tumour_dir},     {"C_value", &A::C_value},                   {"coverage_cutoff", &A::coverage_cutoff},
                                        {"calling_cutoff", &A::calling_cutoff}, {"fdr", &A::fdr},                       {"q_min", &A::q_min},
                                        {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_false_discovery, &A::refbases_file); }
