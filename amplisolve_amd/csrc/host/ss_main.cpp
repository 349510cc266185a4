// AmpliSolveSubstitutionSpectrum -- per-file substitution spectrum and strand asymmetry of the normals and the tumours of a panel against
// the panel of normals, in the reference's key=value style.
//   AmpliSolveSubstitutionSpectrum panel_design=<bed> reference_genome=<fa> germline_dir=<dir> tumour_dir=<dir|-> output_dir=<dir>
//                                  coverage_cutoff=<i> max_alt_pm=<i> min_sites=<i> min_normals=<i> excess_ratio=<f> z_cutoff=<f> asym_delta=<f>
// Exactly 12 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include "main_args.hpp"

using A = ampli::SsArgs;

static const char USAGE[] = "Usage:\n\tAmpliSolveSubstitutionSpectrum panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir or -> "
                            "output_dir=<dir> coverage_cutoff=<int> max_alt_pm=<int> min_sites=<int> min_normals=<int> excess_ratio=<float> z_cutoff=<float> "
                            "asym_delta=<float>\n\tAll arguments are required, in this order (usual values: coverage_cutoff=100 max_alt_pm=30 min_sites=200 "
                            "min_normals=5 excess_ratio=3 z_cutoff=10 asym_delta=0.15).";

static const ampli::KeyArg<A> KEYS[] = {{"panel_design", &A::panel_design}, {"reference_genome", &A::reference_genome}, {"germline_dir", &A::germline_dir},
                                        {"tumour_dir", &A::tumour_dir},     {"output_dir", &A::output_dir},             {"coverage_cutoff", &A::coverage_cutoff},
                                        {"max_alt_pm", &A::max_alt_pm},     {"min_sites", &A::min_sites},               {"min_normals", &A::min_normals},
                                        {"excess_ratio", &A::excess_ratio}, {"z_cutoff", &A::z_cutoff},                 {"asym_delta", &A::asym_delta}};

int main(int argc, char **argv) { return ampli::command_main(argc, argv, USAGE, KEYS, ampli::run_substitution_spectrum, &A::refbases_file); }
