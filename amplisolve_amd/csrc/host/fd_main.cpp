// AmpliSolveFalseDiscovery -- every tumour cell scored against the panel's error table, the Benjamini-Hochberg adjusted score of every
// cell per file, and the cells that pass at a false-discovery rate, in the reference's key=value style.
//   AmpliSolveFalseDiscovery panel_design=<bed> reference_genome=<fa> germline_dir=<dir> tumour_dir=<dir> C_value=<f>
//                            coverage_cutoff=<i> calling_cutoff=<i> fdr=<f> q_min=<f> output_dir=<dir>
// Exactly 10 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 11) {
        std::cout << "Usage:\n\tAmpliSolveFalseDiscovery panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir> "
                     "C_value=<float> coverage_cutoff=<int> calling_cutoff=<int> fdr=<float> q_min=<float> output_dir=<dir>\n"
                     "\tAll arguments are required, in this order (usual values: C_value=0.002 coverage_cutoff=100 calling_cutoff=100 fdr=0.05 "
                     "q_min=13)." << std::endl;
        return 1;
    }
    ampli::FdArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.reference_genome = token(argv[2], "reference_genome");
    a.germline_dir = token(argv[3], "germline_dir");
    a.tumour_dir = token(argv[4], "tumour_dir");
    a.C_value = token(argv[5], "C_value");
    a.coverage_cutoff = token(argv[6], "coverage_cutoff");
    a.calling_cutoff = token(argv[7], "calling_cutoff");
    a.fdr = token(argv[8], "fdr");
    a.q_min = token(argv[9], "q_min");
    a.output_dir = token(argv[10], "output_dir");
    if (const char *e = getenv("AMPLISOLVE_REFBASES_FILE")) a.refbases_file = e; // pre-computed chrom/pos/base table instead of the FASTA
    return ampli::finish(ampli::run_false_discovery(a));
}
