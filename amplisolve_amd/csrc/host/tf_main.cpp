// AmpliSolveTumourFraction -- the tumour fraction of every variant list in every sample: the score estimate, its interval and a verdict,
// the assigned (sample, list) pairs, and the change between consecutive draws of one list, in the reference's key=value
// style.
//   AmpliSolveTumourFraction errorFile=<table> sample_dir=<dir> variants=<file> assign=<file|-> coverage_cutoff=<i> min_variants=<i>
//                            max_vaf=<f> confidence=<0.90|0.95|0.99> output_dir=<dir>
// Exactly 9 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::TfArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveTumourFraction errorFile=<error table> sample_dir=<dir> variants=<file> assign=<file or -> coverage_cutoff=<int> "
                            "min_variants=<int> max_vaf=<float> confidence=<0.90, 0.95 or 0.99> output_dir=<dir>\n"
                            "\tAll arguments are required, in this order (usual values: coverage_cutoff=100 min_variants=5 max_vaf=1 confidence=0.95).\n"
                            "\tvariants: list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt<TAB>weight per line, the weight in (0, 1]: the variant's allele fraction per unit "
                            "of tumour fraction; assign: sample<TAB>list per line, or - for none; consecutive lines that name one list are consecutive draws.";

static const ampli::KeyArg<A> KEYS[] = {{"errorFile", &A::error_file},   {"sample_dir", &A::sample_dir},           {"variants", &A::variants},
                                        {"assign", &A::assign},          {"coverage_cutoff", &A::coverage_cutoff}, {"min_variants", &A::min_variants},
                                        {"max_vaf", &A::max_vaf},        {"confidence", &A::confidence},           {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_tumour_fraction); }
