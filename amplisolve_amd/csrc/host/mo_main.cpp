// AmpliSolveVariantMonitoring -- tumour-informed monitoring: the pooled evidence of every variant list in every sample, every assigned
// (sample, list) pair against matched random control lists, and how often a list "detects" a sample it is not assigned to,
// in the reference's key=value style.
//   AmpliSolveVariantMonitoring errorFile=<table> sample_dir=<dir> variants=<file> assign=<file|-> coverage_cutoff=<i> q_min=<f>
//                               min_variants=<i> min_seen=<i> max_vaf=<f> controls=<i> seed=<u64> output_dir=<dir>
// Exactly 12 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::MoArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveVariantMonitoring errorFile=<error table> sample_dir=<dir> variants=<file> assign=<file or -> coverage_cutoff=<int> "
                            "q_min=<float> min_variants=<int> min_seen=<int> max_vaf=<float> controls=<int> seed=<int> output_dir=<dir>\n"
                            "\tAll arguments are required, in this order (usual values: coverage_cutoff=100 q_min=20 min_variants=5 min_seen=2 max_vaf=1 "
                            "controls=100 seed=1).\n"
                            "\tvariants: list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt per line; assign: sample<TAB>list per line, or - for none.";

static const ampli::KeyArg<A> KEYS[] = {{"errorFile", &A::error_file},       {"sample_dir", &A::sample_dir},     {"variants", &A::variants},
                                        {"assign", &A::assign},              {"coverage_cutoff", &A::coverage_cutoff}, {"q_min", &A::q_min},
                                        {"min_variants", &A::min_variants},  {"min_seen", &A::min_seen},         {"max_vaf", &A::max_vaf},
                                        {"controls", &A::controls},          {"seed", &A::seed},                 {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_variant_monitoring); }
