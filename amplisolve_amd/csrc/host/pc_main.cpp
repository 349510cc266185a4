// AmpliSolvePairedComparison -- two count files of one patient tested against each other at every cell: tumour against matched normal,
// baseline against follow-up, replicate against replicate, in the reference's key=value style.
//   AmpliSolvePairedComparison panel_design=<bed> reference_genome=<fa> sample_dir=<dir> pairs=<file> depth_cutoff=<i> q_min=<f>
//                              min_vaf=<f> output_dir=<dir>
// Exactly 8 tokens in this order.  pairs: nameA<TAB>nameB per line, the names as the Summary names samples.  Not a drop-in: the exit
// status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 9) {
        std::cout << "Usage:\n\tAmpliSolvePairedComparison panel_design=<bed> reference_genome=<fasta> sample_dir=<dir> pairs=<file> depth_cutoff=<int> "
                     "q_min=<float> min_vaf=<float> output_dir=<dir>\n"
                     "\tAll arguments are required, in this order (usual values: depth_cutoff=100 q_min=13 min_vaf=0.005; pairs lists nameA<TAB>nameB per "
                     "line)." << std::endl;
        return 1;
    }
    ampli::PcArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.reference_genome = token(argv[2], "reference_genome");
    a.sample_dir = token(argv[3], "sample_dir");
    a.pairs = token(argv[4], "pairs");
    a.depth_cutoff = token(argv[5], "depth_cutoff");
    a.q_min = token(argv[6], "q_min");
    a.min_vaf = token(argv[7], "min_vaf");
    a.output_dir = token(argv[8], "output_dir");
    if (const char *e = getenv("AMPLISOLVE_REFBASES_FILE")) a.refbases_file = e; // pre-computed chrom/pos/base table instead of the FASTA
    return ampli::finish(ampli::run_paired_comparison(a));
}
