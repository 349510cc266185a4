// AmpliSolveSampleConcordance -- sample identity of the normals and the tumours of a panel from their counts alone, in
// the reference's key=value style.
//   AmpliSolveSampleConcordance panel_design=<bed> germline_dir=<dir> tumour_dir=<dir|-> min_depth=<i> min_sites=<i> same_fraction=<f> output_dir=<dir>
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
        std::cout << "Usage:\n\tAmpliSolveSampleConcordance panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> min_depth=<int> "
                     "min_sites=<int> same_fraction=<float> output_dir=<dir>\n\tAll arguments are required, in this order." << std::endl;
        return 1;
    }
    ampli::ScArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.germline_dir = token(argv[2], "germline_dir");
    a.tumour_dir = token(argv[3], "tumour_dir");
    a.min_depth = token(argv[4], "min_depth");
    a.min_sites = token(argv[5], "min_sites");
    a.same_fraction = token(argv[6], "same_fraction");
    a.output_dir = token(argv[7], "output_dir");
    return ampli::finish(ampli::run_sample_concordance(a));
}
