// AmpliSolveAllelicImbalance -- the allelic balance of every file at the het sites of its germline, against the share the panel of normals
// shows there, pooled per gene, in the reference's key=value style.
//   AmpliSolveAllelicImbalance panel_design=<bed> germline_dir=<dir> tumour_dir=<dir|-> pairs=<file|self> output_dir=<dir> min_depth=<i>
//                              min_normals=<i> site_q=<f> min_sites=<i> q_min=<f> min_imbalance=<f>
// Exactly 11 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::AiArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveAllelicImbalance panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> pairs=<file or self> output_dir=<dir> "
                            "min_depth=<int> min_normals=<int> site_q=<float> min_sites=<int> q_min=<float> min_imbalance=<float>\n"
                            "\tAll arguments are required, in this order (usual values: min_depth=100 min_normals=5 site_q=20 min_sites=3 q_min=20 "
                            "min_imbalance=0.02).\n"
                            "\ttumour_dir=-: the normals again (the null calibration); pairs: tumourName<TAB>normalName per line, or self.";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design}, {"germline_dir", &A::germline_dir}, {"tumour_dir", &A::tumour_dir},
                                        {"pairs", &A::pairs},               {"output_dir", &A::output_dir},     {"min_depth", &A::min_depth},
                                        {"min_normals", &A::min_normals},   {"site_q", &A::site_q},             {"min_sites", &A::min_sites},
                                        {"q_min", &A::q_min},               {"min_imbalance", &A::min_imbalance}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_allelic_imbalance); }
