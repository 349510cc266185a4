// AmpliSolveInSilicoDilution -- an in-silico dilution series: count files mixed read by read on the device at the listed fractions, every
// mixture gated with the error table's thresholds, the share of the source's calls still found beside the predicted power,
// in the reference's key=value style.
//   AmpliSolveInSilicoDilution errorFile=<error table> sample_dir=<dir> mixtures=<file> replicates=<i> seed=<u64> coverage_cutoff=<i>
//                              confidence=<f> write_counts=<0|1> output_dir=<dir>
// Exactly 9 tokens in this order.  mixtures: source<TAB>diluent<TAB>fraction[<TAB>scale] per line, the names as the Summary names samples,
// diluent - for none.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::DiArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveInSilicoDilution errorFile=<error table> sample_dir=<dir> mixtures=<file> replicates=<int> seed=<int> "
                            "coverage_cutoff=<int> confidence=<0.5 .. 0.99> write_counts=<0 or 1> output_dir=<dir>\n"
                            "\tAll arguments are required, in this order (usual values: replicates=8 seed=1 coverage_cutoff=100 confidence=0.95 write_counts=0; "
                            "mixtures lists source<TAB>diluent<TAB>fraction[<TAB>scale] per line, diluent - for none).";

static const ampli::KeyArg<A> KEYS[] = {{"errorFile", &A::error_file},   {"sample_dir", &A::sample_dir},           {"mixtures", &A::mixtures},
                                        {"replicates", &A::replicates},  {"seed", &A::seed},                       {"coverage_cutoff", &A::coverage_cutoff},
                                        {"confidence", &A::confidence},  {"write_counts", &A::write_counts},       {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_insilico_dilution); }
