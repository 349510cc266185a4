// computeIndelCounts -- BAM -> <out>/<sample>.INDEL.PILEUP.ASEQ + <out>/<sample>.INDEL.LENGTHS.txt: per listed position
// and read strand, how many reads show an insertion, a deletion or neither at the junction behind that position, as a count file
// that every command reads like a substitution count file (reference base A everywhere, A>C = insertion, A>G = deletion).
//   computeIndelCounts vcf=<positions> bam=<file.bam> threads=<int> mbq=<int> mrq=<int> mdc=<int> refbases=<path> out=<dir>
// key=value tokens as computeCounts takes them; vcf, bam and out are required, the rest default to 4 / 20 / 20 / 20 / none.
// Exit status: 0 on success, 1 on failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "host.hpp"

int main(int argc, char **argv)
{
    ampli::CiArgs a;
    bool bad = argc < 2;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { bad = true; continue; }
        const std::string key(argv[i], eq - argv[i]), val(eq + 1);
        if (key == "vcf") a.vcf = val;
        else if (key == "bam") a.bam = val;
        else if (key == "out") a.out_dir = val;
        else if (key == "refbases") a.refbases = val;
        else if (key == "threads") a.threads = atoi(val.c_str());
        else if (key == "mbq") a.mbq = atoi(val.c_str());
        else if (key == "mrq") a.mrq = atoi(val.c_str());
        else if (key == "mdc") a.mdc = atoi(val.c_str());
        else bad = true;
    }
    if (bad || a.vcf.empty() || a.bam.empty() || a.out_dir.empty()) {
        std::cout << "Usage:\n\tcomputeIndelCounts vcf=<dummyVCF.txt> bam=<file.bam> [threads=<int>] [mbq=<int>] [mrq=<int>] [mdc=<int>] [refbases=<path>] out=<dir>\n"
                     "\tvcf: every position of the panel, one per line (chr pos ...); mbq / mrq / mdc: minimum quality of the base in front of the\n"
                     "\tjunction, read (mapping) quality and depth of coverage (20 20 20 recommended); writes <out>/<bam name>.INDEL.PILEUP.ASEQ\n"
                     "\t(ref A everywhere: A = reads with neither, C = reads with an insertion, G = reads with a deletion behind the position) and\n"
                     "\t<out>/<bam name>.INDEL.LENGTHS.txt (chr pos INS|DEL len count; len 32 means >= 32); refbases: also write the table\n"
                     "\t`chrom pos A` to hand to the commands as AMPLISOLVE_REFBASES_FILE.  out must not be the directory of the substitution\n"
                     "\tcount files: the commands take every *.ASEQ file of a directory" << std::endl;
        return 1;
    }
    return ampli::run_compute_indel_counts(a) ? 1 : 0;
}
