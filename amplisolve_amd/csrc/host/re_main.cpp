// computeReadEvidence -- BAM + a list of calls -> <out>/<sample>.EVIDENCE.txt + <out>/<sample>.EVIDENCE.HIST.txt: for every
// listed call, do the reads that carry the alt allele rank below the reads that carry the ref allele in base quality, MAPQ or distance to
// the end of the read (what other callers print as BaseQRankSum, MQRankSum and ReadPosRankSum).
//   computeReadEvidence vcf=<calls> bam=<file.bam> threads=<int> mbq=<int> mrq=<int> min_alt=<int> z_min=<decimal> out=<dir>
// key=value tokens as computeCounts takes them; vcf, bam and out are required, the rest default to 4 / 20 / 20 / 4 / 3.
// Exit status: 0 on success, 1 on failure.
#include <cstring>
#include <iostream>

#include "host.hpp"

int main(int argc, char **argv)
{
    ampli::ReArgs a;
    bool bad = argc < 2;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { bad = true; continue; }
        const std::string key(argv[i], eq - argv[i]), val(eq + 1);
        if (key == "vcf") a.vcf = val;
        else if (key == "bam") a.bam = val;
        else if (key == "out") a.out_dir = val;
        else if (key == "threads") a.threads = val;
        else if (key == "mbq") a.mbq = val;
        else if (key == "mrq") a.mrq = val;
        else if (key == "min_alt") a.min_alt = val;
        else if (key == "z_min") a.z_min = val;
        else bad = true;
    }
    if (bad || a.vcf.empty() || a.bam.empty() || a.out_dir.empty()) {
        std::cout << "Usage:\n\tcomputeReadEvidence vcf=<calls.txt> bam=<file.bam> [threads=<int>] [mbq=<int>] [mrq=<int>] [min_alt=<int>] [z_min=<decimal>] out=<dir>\n"
                     "\tvcf: the calls to examine, one per line (chr pos id ref alt); ref and alt select the two alleles, an alt of . takes the\n"
                     "\tnon-reference base with the most reads, a multi-base or non-ACGT ref or alt leaves the line UNTESTED.  List calls, not the\n"
                     "\tpanel: every listed position keeps 3 KB of bins, a sparse list is counted in on-chip memory, and a list of every panel\n"
                     "\tposition takes the slow path of one memory update per base and metric (measured: twelve times the time of computeCounts).\n"
                     "\tmbq / mrq: minimum base quality and read (mapping) quality, as computeCounts (20 20); min_alt: the reads either allele\n"
                     "\tneeds for a verdict (an integer >= 1, default 4); z_min: the score from which a metric is flagged (a decimal > 0, default 3).\n"
                     "\tWrites <out>/<bam name>.EVIDENCE.txt (chr pos ref alt n_ref n_alt, then med_ref med_alt z for base quality, MAPQ / 4 and\n"
                     "\tdistance to the read's nearer end, then UNTESTED, PASS or a comma-joined subset of LOW_BQ LOW_MQ READ_END; z < 0: the alt\n"
                     "\treads rank below the ref reads) and <out>/<bam name>.EVIDENCE.HIST.txt (chr pos nt metric bin count per non-zero bin)" << std::endl;
        return 1;
    }
    return ampli::run_compute_read_evidence(a) ? 1 : 0;
}
