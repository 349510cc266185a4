// AmpliSolveNormalExceedance -- how many normals of the panel show an allele at a tumour's fraction or above, and the cells that top
// (nearly) all of them on both strands, in the reference's key=value style.
//   AmpliSolveNormalExceedance panel_design=<bed> reference_genome=<fa> germline_dir=<dir> tumour_dir=<dir|-> output_dir=<dir>
//                              coverage_cutoff=<i> calling_cutoff=<i> min_alt_reads=<i> min_vaf_pm=<i> min_normals=<i> max_normals=<i>
// Exactly 11 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 12) {
        std::cout << "Usage:\n\tAmpliSolveNormalExceedance panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir or -> "
                     "output_dir=<dir> coverage_cutoff=<int> calling_cutoff=<int> min_alt_reads=<int> min_vaf_pm=<int> min_normals=<int> max_normals=<int>\n"
                     "\tAll arguments are required, in this order (usual values: coverage_cutoff=100 calling_cutoff=100 min_alt_reads=3 min_vaf_pm=0 "
                     "min_normals=10 max_normals=0)." << std::endl;
        return 1;
    }
    ampli::ExArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.reference_genome = token(argv[2], "reference_genome");
    a.germline_dir = token(argv[3], "germline_dir");
    a.tumour_dir = token(argv[4], "tumour_dir");
    a.output_dir = token(argv[5], "output_dir");
    a.coverage_cutoff = token(argv[6], "coverage_cutoff");
    a.calling_cutoff = token(argv[7], "calling_cutoff");
    a.min_alt_reads = token(argv[8], "min_alt_reads");
    a.min_vaf_pm = token(argv[9], "min_vaf_pm");
    a.min_normals = token(argv[10], "min_normals");
    a.max_normals = token(argv[11], "max_normals");
    if (const char *e = getenv("AMPLISOLVE_REFBASES_FILE")) a.refbases_file = e; // pre-computed chrom/pos/base table instead of the FASTA
    return ampli::finish(ampli::run_normal_exceedance(a));
}
