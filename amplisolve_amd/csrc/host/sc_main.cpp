// AmpliSolveSampleConcordance -- sample identity of the normals and the tumours of a panel from their counts alone, in
// the reference's key=value style.
//   AmpliSolveSampleConcordance panel_design=<bed> germline_dir=<dir> tumour_dir=<dir|-> min_depth=<i> min_sites=<i> same_fraction=<f> output_dir=<dir>
// Exactly 7 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::ScArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveSampleConcordance panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> min_depth=<int> "
                            "min_sites=<int> same_fraction=<float> output_dir=<dir>\n\tAll arguments are required, in this order.";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design}, {"germline_dir", &A::germline_dir},   {"tumour_dir", &A::tumour_dir},
                                        {"min_depth", &A::min_depth},       {"min_sites", &A::min_sites},         {"same_fraction", &A::same_fraction},
                                        {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_sample_concordance); }
