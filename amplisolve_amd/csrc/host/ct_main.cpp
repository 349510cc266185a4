// AmpliSolveContamination -- cross-sample contamination among the normals and the tumours of a panel from their counts alone
// (DESIGN 15), in the reference's key=value style.
//   AmpliSolveContamination panel_design=<bed> germline_dir=<dir> tumour_dir=<dir|-> output_dir=<dir> min_depth=<i> min_sites=<i> min_fraction=<f>
// Exactly 7 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::CtArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveContamination panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> output_dir=<dir> "
                            "min_depth=<int> min_sites=<int> min_fraction=<float>\n\tAll arguments are required, in this order "
                            "(usual values: min_depth=100 min_sites=20 min_fraction=0.005).";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design}, {"germline_dir", &A::germline_dir}, {"tumour_dir", &A::tumour_dir},
                                        {"output_dir", &A::output_dir},     {"min_depth", &A::min_depth},       {"min_sites", &A::min_sites},
                                        {"min_fraction", &A::min_fraction}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_contamination); }
