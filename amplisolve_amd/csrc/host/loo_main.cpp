// AmpliSolveLeaveOneOut -- the leave-one-out false-call check of a panel of normals, in the reference's key=value style.
//   AmpliSolveLeaveOneOut panel_design=<bed> reference_genome=<fa> germline_dir=<dir> C_value=<f>[,<f>...] coverage_cutoff=<i>
//                         calling_cutoff=<i> output_dir=<dir>
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
        std::cout << "Usage:\n\tAmpliSolveLeaveOneOut panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> C_value=<float>[,<float>...] "
                     "coverage_cutoff=<int> calling_cutoff=<int> output_dir=<dir>\n\tAll arguments are required, in this order." << std::endl;
        return 1;
    }
    ampli::LooArgs a;
    a.panel_design = token(argv[1], "panel_design");
    a.reference_genome = token(argv[2], "reference_genome");
    a.germline_dir = token(argv[3], "germline_dir");
    a.C_value = token(argv[4], "C_value");
    a.coverage_cutoff = token(argv[5], "coverage_cutoff");
    a.calling_cutoff = token(argv[6], "calling_cutoff");
    a.output_dir = token(argv[7], "output_dir");
    if (const char *e = getenv("AMPLISOLVE_REFBASES_FILE")) a.refbases_file = e;
    return ampli::finish(ampli::run_leave_one_out(a));
}
