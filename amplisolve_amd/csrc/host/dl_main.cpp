// AmpliSolveDetectionLimit -- per-sample detection limits of the calling gate, in the reference's key=value style.
//   AmpliSolveDetectionLimit errorFile=<table> tumour_dir=<dir> output_dir=<dir> coverage_cutoff=<int> levels=<f>[,<f>...]
// Exactly 5 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::DlArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveDetectionLimit errorFile=<error table> tumour_dir=<dir> output_dir=<dir> coverage_cutoff=<int> "
                            "levels=<float>[,<float>...]\n\tAll arguments are required, in this order.";

static const ampli::KeyArg<A> KEYS[] = {{"errorFile", &A::error_file},
                                        {"tumour_dir", &A::tumour_dir},
                                        {"output_dir", &A::output_dir},
                                        {"coverage_cutoff", &A::coverage_cutoff},
                                        {"levels", &A::levels}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_detection_limits); }
