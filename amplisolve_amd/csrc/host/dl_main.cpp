// AmpliSolveDetectionLimit -- per-sample detection limits of the calling gate, in the reference's key=value style.
//   AmpliSolveDetectionLimit errorFile=<table> tumour_dir=<dir> output_dir=<dir> coverage_cutoff=<int> levels=<f>[,<f>...]
// Exactly 5 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 6) {
        std::cout << "Usage:\n\tAmpliSolveDetectionLimit errorFile=<error table> tumour_dir=<dir> output_dir=<dir> coverage_cutoff=<int> "
                     "levels=<float>[,<float>...]\n\tAll arguments are required, in this order." << std::endl;
        return 1;
    }
    ampli::DlArgs a;
    a.error_file = token(argv[1], "errorFile");
    a.tumour_dir = token(argv[2], "tumour_dir");
    a.output_dir = token(argv[3], "output_dir");
    a.coverage_cutoff = token(argv[4], "coverage_cutoff");
    a.levels = token(argv[5], "levels");
    return ampli::finish(ampli::run_detection_limits(a));
}
