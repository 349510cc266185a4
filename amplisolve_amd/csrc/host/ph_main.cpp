// computePhasing -- BAM + a list of calls -> <out>/<sample>.PHASE.txt + <out>/<sample>.PHASE.MNV.txt: for every two listed calls
// at most max_dist apart, which alleles the reads that cover both show at both -- are the two one event (CIS), on different molecules
// (TRANS), or is one the other's subset.
//   computePhasing vcf=<calls> bam=<file.bam> threads=<int> mbq=<int> mrq=<int> min_alt=<int> min_share=<int> q_min=<decimal> max_dist=<int> out=<dir>
// key=value tokens as computeCounts takes them; vcf, bam and out are required, the rest default to 4 / 20 / 20 / 4 / 10 / 13 / 200.
// Exit status: 0 on success, 1 on failure.
#include <cstring>
#include <iostream>

#include "host.hpp"

int main(int argc, char **argv)
{
    ampli::PhArgs a;
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
        else if (key == "min_share") a.min_share = val;
        else if (key == "q_min") a.q_min = val;
        else if (key == "max_dist") a.max_dist = val;
        else bad = true;
    }
    if (bad || a.vcf.empty() || a.bam.empty() || a.out_dir.empty()) {
        std::cout << "Usage:\n\tcomputePhasing vcf=<calls.txt> bam=<file.bam> [threads=<int>] [mbq=<int>] [mrq=<int>] [min_alt=<int>] [min_share=<int>] [q_min=<decimal>]\n"
                     "\t               [max_dist=<int>] out=<dir>\n"
                     "\tvcf: the calls to pair, one per line (chr pos id ref alt).  Every two lines on one chromosome at most max_dist apart (an integer\n"
                     "\t>= 1, default 200) are a pair; lines at the same position are none.  Alignment records are counted, not fragments: overlapping\n"
                     "\tmates count twice, as in computeCounts.  Only the next 8 listed positions are partners: a pair further apart in the list is\n"
                     "\twritten as NOT_FORMED.  Strands are pooled.  An insertion has no position of its own; a multi-base or non-ACGT ref or alt\n"
                     "\tleaves the pair UNTESTED.  List calls, not the panel: a list of every panel position takes\n"
                     "\tthe slow path of one memory update per read and pair (measured: 1.2 times computeReadEvidence on such a list).\n"
                     "\tmbq / mrq: minimum base quality and read (mapping) quality, as computeCounts (20 20).  A group of reads (alt at both, alt at A\n"
                     "\tonly, alt at B only) is present with min_alt reads (an integer >= 1, default 4) that are min_share per cent (0 .. 100, default\n"
                     "\t10) of the reads with an alt at either.  Verdicts: CIS (only alt at both), NESTED_B / NESTED_A (B's / A's alt reads are a subset\n"
                     "\tof the other's), each with the exact test's score >= q_min (a decimal > 0, default 13), else UNRESOLVED; TRANS (never alt at\n"
                     "\tboth), MIXED (all three groups), UNTESTED (a variant without reads among the joint ones).  TRANS and MIXED carry no score\n"
                     "\tgate: at low allele fractions the absence of reads with both alts is not significant as an association; exp_aa beside it\n"
                     "\tsays how many were expected.\n"
                     "\tWrites <out>/<bam name>.PHASE.txt (chr posA refA altA posB refB altB n_joint n_rr n_ra n_ar n_aa n_other exp_aa score verdict;\n"
                     "\tthe first letter is the allele at A; score > 0: linked in cis) and <out>/<bam name>.PHASE.MNV.txt (chr pos ref_string\n"
                     "\talt_string reads per chain of 2 or 3 consecutive positions that are CIS in pairs)" << std::endl;
        return 1;
    }
    return ampli::run_compute_phasing(a) ? 1 : 0;
}
