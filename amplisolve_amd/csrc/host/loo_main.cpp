// AmpliSolveLeaveOneOut -- the leave-one-out false-call check of a panel of normals, in the reference's key=value style.
//   AmpliSolveLeaveOneOut panel_design=<bed> reference_genome=<fa> germline_dir=<dir> C_value=<f>[,<f>...] coverage_cutoff=<i>
//                         calling_cutoff=<i> output_dir=<dir>
// Exactly 7 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::LooArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveLeaveOneOut panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> C_value=<float>[,<float>...] "
                            "coverage_cutoff=<int> calling_cutoff=<int> output_dir=<dir>\n\tAll arguments are required, in this order.";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design},       {"reference_genome", &A::reference_genome},
                                        {"germline_dir", &A::germline_dir},       {"C_value", &A::C_value},
                                        {"coverage_cutoff", &A::coverage_cutoff}, {"calling_cutoff", &A::calling_cutoff},
                                        {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_leave_one_out, &A::refbases_file); }
