// AmpliSolveContamination -- cross-sample contamination among the normals and the tumours of a panel from their counts alone
// (DESIGN 15), in the reference's key=value style.
//   AmpliSolveContamination panel_design=<bed> germline_dir=<dir> tumour_dir=<dir|-> output_dir=<dir> min_depth=<i> min_sites=<i> min_fraction=<f>
// Exactly 7 tokens in this order.  Not a drop-in: the exit status is 0 on success and 1 on any failure.
#include <clocale>
#include <cstdlib>

#include "host.hpp"
#include "main_args.hpp"

using ampli::token;

int main(int argc, char **argv)
{
    setlocale(LC_ALL, "");
    if (argc != 8) {
        std::cout << "Usage:\n\tAmpliSolveContamination panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> output_dir=<dir> "
                     "min_depth=<int> min_sites=<int> min_fraction=<float>\n\tAll arguments are required, in this order "
                     "(usual values: min_depth=100 min_sites=20 min_fraction=0.005)." << std::endl;
        return 1;
    }
    ampli::CtArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.germline_dir = token(argv[2], "germline_dir");
    a.tumour_dir = token(argv[3], "tumour_dir");
    a.output_dir = token(argv[4], "output_dir");
    a.min_depth = token(argv[5], "min_depth");
    a.min_sites = token(argv[6], "min_sites");
    a.min_fraction = token(argv[7], "min_fraction");
    return ampli::finish(ampli::run_contamination(a));
}
