// AmpliSolveInSilicoDilution -- an in-silico dilution series: count files mixed read by read on the device at the listed fractions, every
// mixture gated with the error table's thresholds, the share of the source's calls still found beside the predicted power,
// in the reference's key=value style.
//   AmpliSolveInSilicoDilution errorFile=<error table> sample_dir=<dir> mixtures=<file> replicates=<i> seed=<u64> coverage_cutoff=<i>
//                              confidence=<f> write_counts=<0|1> output_dir=<dir>
// Exactly 9 tokens in this order.  mixtures: source<TAB>diluent<TAB>fraction[<TAB>scale] per line, the names as the Summary names samples,
// diluent - for none.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 10) {
        std::cout << "Usage:\n\tAmpliSolveInSilicoDilution errorFile=<error table> sample_dir=<dir> mixtures=<file> replicates=<int> seed=<int> "
                     "coverage_cutoff=<int> confidence=<0.5 .. 0.99> write_counts=<0 or 1> output_dir=<dir>\n"
                     "\tAll arguments are required, in this order (usual values: replicates=8 seed=1 coverage_cutoff=100 confidence=0.95 write_counts=0; "
                     "mixtures lists source<TAB>diluent<TAB>fraction[<TAB>scale] per line, diluent - for none)." << std::endl;
        return 1;
    }
    ampli::DiArgs a;
    a.error_file = token(argv[1], "errorFile");
    a.sample_dir = token(argv[2], "sample_dir");
    a.mixtures = token(argv[3], "mixtures");
    a.replicates = token(argv[4], "replicates");
    a.seed = token(argv[5], "seed");
    a.coverage_cutoff = token(argv[6], "coverage_cutoff");
    a.confidence = token(argv[7], "confidence");
    a.write_counts = token(argv[8], "write_counts");
    a.output_dir = token(argv[9], "output_dir");
    return ampli::finish(ampli::run_insilico_dilution(a));
}
