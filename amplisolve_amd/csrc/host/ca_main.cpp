// computeAmpliconCounts -- BAM + BED -> <out>/<sample>.AMPLICON.PILEUP.ASEQ, .AMPLICON.READS.txt, .AMPLICON.OVERLAPS.txt: every
// read is assigned to the amplicon it came from and counted inside that amplicon only; a position under two amplicons keeps both counts.
//   computeAmpliconCounts vcf=<positions> bam=<file.bam> bed=<panel.bed> threads=<int> mbq=<int> mrq=<int> mdc=<int> min_overlap=<int>
//                         layers=<dir> out=<dir>
// key=value tokens as computeCounts takes them; vcf, bam, bed and out are required, the rest default to 4 / 20 / 20 / 20 / 50 / none.
// Exit status: 0 on success, 1 on failure.
#include <cstring>
#include <iostream>

#include "host.hpp"

int main(int argc, char **argv)
{
    ampli::CaArgs a;
    bool bad = argc < 2;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { bad = true; continue; }
        const std::string key(argv[i], eq - argv[i]), val(eq + 1);
        if (key == "vcf") a.vcf = val;
        else if (key == "bam") a.bam = val;
        else if (key == "bed") a.bed = val;
        else if (key == "out") a.out_dir = val;
        else if (key == "layers") a.layers_dir = val;
        else if (key == "threads") a.threads = val;
        else if (key == "mbq") a.mbq = val;
        else if (key == "mrq") a.mrq = val;
        else if (key == "mdc") a.mdc = val;
        else if (key == "min_overlap") a.min_overlap = val;
        else bad = true;
    }
    if (bad || a.vcf.empty() || a.bam.empty() || a.bed.empty() || a.out_dir.empty()) {
        std::cout << "Usage:\n\tcomputeAmpliconCounts vcf=<dummyVCF.txt> bam=<file.bam> bed=<panel.bed> [threads=<int>] [mbq=<int>] [mrq=<int>] [mdc=<int>]\n"
                     "\t                      [min_overlap=<int>] [layers=<dir>] out=<dir>\n"
                     "\tvcf: every position of the panel, one per line (chr pos ...); bed: the panel's amplicons (chrom start end name . gene);\n"
                     "\tmbq / mrq / mdc: minimum base quality, read (mapping) quality and depth of coverage (20 20 20 recommended); min_overlap:\n"
                     "\tthe share of a read's span, in percent (1 .. 100, default 50), that must lie inside its amplicon.  Every read is assigned to\n"
                     "\tone amplicon and counted inside it only.  Writes <out>/<bam name>.AMPLICON.PILEUP.ASEQ (the sum over the amplicons that\n"
                     "\tcover a position), <out>/<bam name>.AMPLICON.READS.txt (reads per BED row, then #kept #assigned #off_target #bases_counted\n"
                     "\t#bases_clipped) and <out>/<bam name>.AMPLICON.OVERLAPS.txt (chr pos name A C G T Ars Crs Grs Trs per amplicon over a\n"
                     "\tposition under two or more).  layers: also write <layers>/<bam name>.AMP1.PILEUP.ASEQ and .AMP2.PILEUP.ASEQ (the first and\n"
                     "\tthe second amplicon over a position) and <layers>/<bam name>.pairs.txt for AmpliSolvePairedComparison.  layers must differ\n"
                     "\tfrom out, and out must not be the directory of the pooled count files: the commands take every *.ASEQ file of a directory" << std::endl;
        return 1;
    }
    return ampli::run_compute_amplicon_counts(a) ? 1 : 0;
}
