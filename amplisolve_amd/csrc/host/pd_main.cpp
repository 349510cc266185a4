// AmpliSolvePanelDispersion -- per-position dispersion of a panel of normals and per-normal outlier scores, in the
// reference's key=value style.
//   AmpliSolvePanelDispersion panel_design=<bed> reference_genome=<fa> germline_dir=<dir> coverage_cutoff=<i> z_cutoff=<f> output_dir=<dir>
// Exactly 6 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::PdArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolvePanelDispersion panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> coverage_cutoff=<int> "
                            "z_cutoff=<float> output_dir=<dir>\n\tAll arguments are required, in this order.";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design}, {"reference_genome", &A::reference_genome},
                                        {"germline_dir", &A::germline_dir}, {"coverage_cutoff", &A::coverage_cutoff},
                                        {"z_cutoff", &A::z_cutoff},         {"output_dir", &A::output_dir}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_panel_dispersion, &A::refbases_file); }
