// AmpliSolveDetectionPower -- detection power at given allele fractions and the limit of detection per (line, base) pair,
// in the reference's key=value style.
//   AmpliSolveDetectionPower errorFile=<table> tumour_dir=<dir> output_dir=<dir> coverage_cutoff=<int> levels=<f>[,<f>...] confidence=<f>
// Exactly 6 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::DpArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveDetectionPower errorFile=<error table> tumour_dir=<dir> output_dir=<dir> coverage_cutoff=<int> "
                            "levels=<float>[,<float>...] confidence=<0.5 .. 0.99>\n\tAll arguments are required, in this order.";

static const ampli::KeyArg<A> KEYS[] = {{"errorFile", &A::error_file}, {"tumour_dir", &A::tumour_dir}, {"output_dir", &A::output_dir},
                                        {"coverage_cutoff", &A::coverage_cutoff}, {"levels", &A::levels}, {"confidence", &A::confidence}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_detection_power); }
