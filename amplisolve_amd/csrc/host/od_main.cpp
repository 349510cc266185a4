// AmpliSolveOverdispersedCalling -- the dispersion of every cell of the panel of normals, every tumour cell scored under the Poisson law
// and under the negative binomial, and the cells that pass the first gate and not the second, in the reference's key=value
// style.
//   AmpliSolveOverdispersedCalling panel_design=<bed> reference_genome=<fa> germline_dir=<dir> tumour_dir=<dir> C_value=<f>
//                                  coverage_cutoff=<i> calling_cutoff=<i> z_cutoff=<f> q_min=<f> output_dir=<dir>
// Exactly 10 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::OdArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveOverdispersedCalling panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir> "
                            "C_value=<float> coverage_cutoff=<int> calling_cutoff=<int> z_cutoff=<float> q_min=<float> output_dir=<dir>\n"
                            "\tAll arguments are required, in this order (usual values: C_value=0.002 coverage_cutoff=100 calling_cutoff=100 z_cutoff=4 "
                            "q_min=13).";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design}, {"reference_genome", &A::reference_genome}, {"germline_dir", &A::germline_dir},
                                        {"tumour_dir", &A::tumour_dir},     {"C_value", &A::C_value},                   {"coverage_cutoff", &A::coverage_cutoff},
                                        {"calling_cutoff", &A::calling_cutoff}, {"z_cutoff", &A::z_cutoff},             {"q_min", &A::q_min},
                                        {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_overdispersed_calling, &A::refbases_file); }
