// amplisolve_amd/csrc/host/run_vc.cpp -- run_variant_calling re-states main() + callVariants of AmpliSolveVariantCalling.cpp
// (VC:199-360, VC:633-3304)
#include "pipeline.hpp"

namespace ampli {

namespace {
struct CallRow : CallBase { double q_fw, q_bw; int flags; }; // flags: AMPLI_CALL_*

// Annotation of one emitted call (Fisher, context, flags: VC:902-1034) and its two text rows: the Summary line and the VCF line.
// first_ever: the first row EVER written to the Summary, which prints its AF columns with the stream's default 6 digits (VC:1066);
// fisher_off: AMPLISOLVE_FISHER=off (run_variant_calling).
std::pair<std::string, std::string> annotate_row(const CallRow &c, const Panel &panel, const std::string &sample_name, float p_value, bool fisher_off,
                                                 bool first_ever)
{
    thread_local std::ostringstream output, vcf; // one pair per annotating thread, emptied for every row
    output.str(std::string());
    vcf.str(std::string());
    output << std::setprecision(first_ever ? 6 : 4);
    const int64_t p = c.p;
    const std::string &chrom = panel.chroms[panel.pos_chrom[p]];
    const int pos = panel.pos_coord[p];
    const int FW = c.fw, BW = c.bw, RD = c.rd; // VC:760-761 and the RD column
    const int alt_fw = c.k_fw, alt_bw = c.k_bw;
    const char refc = "ACGT"[panel.ref_code[p]], altc = "ACGT"[c.alt];
    const std::string Flag_Dup = panel.dup[p] ? "YES" : "NO";
    const double pf = fisher_off ? -1 : fisher_two_sided(RD - BW, BW, alt_fw, alt_bw); // VC:901-902
    const std::string Flag_Fisher = pf <= p_value ? "YES" : "NO";         // VC:903-910
    const std::string Flag_Tier = (alt_fw < 5 || alt_bw < 5) ? "LowQual" : "HighQual"; // VC:912-919
    const std::string GermlineFlag = "-";                                 // VC:927-935 (map holds a dummy entry only)
    const std::string MaxGermlineFlag = panel.germ_cell(c.alt, p);        // VC:943-954
    const std::string down = kmer_down(panel, chrom, pos), up = kmer_up(panel, chrom, pos);
    const double Q = (c.q_fw + c.q_bw) / 2.000;                           // VC:968
    const std::string cat = Flag_Dup + "_" + Flag_Fisher;
    const double max_germ = std::atof(MaxGermlineFlag.c_str());           // VC:972
    const int homo = homopolymer_test(down, up, altc);
    // VC:993-1034: flags go through an unordered_map and come out in ITS order
    std::unordered_map<std::string, std::string> Flag_Hash;
    int OK = 0;
    auto put = [&](const char *f) { OK = 1; Flag_Hash.insert(std::make_pair<std::string, std::string>(f, f)); };
    if (cat == "YES_NO") put("AmpliconEdge");
    if (cat == "YES_YES") put("AmpliconEdge;StrandBias");
    if (cat == "NO_YES") put("StrandBias");
    if (c.af < max_germ && cat == "NO_NO" && Flag_Tier != "HighQual") put("PositionWithHighNoise");
    if (homo == 1) put("HomoPolymerRegion");
    if (c.q_fw < 20 || c.q_bw < 20) put("LowQ");
    if (Flag_Tier != "HighQual") put("LowSupportingReads");
    std::string filter = "PASS";
    if (OK) {
        filter.clear();
        for (auto it = Flag_Hash.begin(); it != Flag_Hash.end(); ++it) filter += (filter.empty() ? "" : ";") + it->first;
    }
    // the C->G block writes "-" instead of "." as ID when the call is not a PASS (VC:1856)
    const char *id = (!OK || !(refc == 'C' && altc == 'G')) ? "." : "-";
    vcf << chrom << "\t" << pos << "\t" << id << "\t" << refc << "\t" << altc << "\t" << Q << "\t" << filter << "\t" << c.af << ";" << RD
        << ";" << alt_fw + alt_bw << "\n"; // VC:1040 / 1062
    // VC:1066 -- std::setprecision(4) is set mid-row and sticks for every later row of the file
    output << sample_name << "\t" << chrom << "\t" << pos << "\t" << refc << "->" << altc << "\t" << RD << "\t" << FW << "\t" << BW << "\t"
           << c.af << "\t" << alt_fw << "\t" << alt_bw << "\t" << c.af_fw << "\t" << c.af_bw << "\t" << Flag_Dup << "_" << Flag_Fisher
           << "\t" << pf << "\t" << std::setprecision(4) << c.q_fw << "\t" << std::setprecision(4) << c.q_bw << "\t" << Flag_Tier << "\t"
           << GermlineFlag << "\t" << MaxGermlineFlag << "\t" << down << "\t" << up << "\t" << homo << "\n";
    return {output.str(), vcf.str()};
}
} // namespace

int run_variant_calling(const VcArgs &a)
{
    try {
        float p_value = (float)std::atof(a.p_value.c_str()); // VC:262-294
        int cov = std::atoi(a.coverage_cutoff.c_str());
        std::cout << kLine << "\n" << std::endl;
        std::cout << "                          AmpliSolve variant calling for batch execution of multiple samples\n" << std::endl;
        std::cout << "                       MI355X-native build (amplisolve_amd); command line and files as AmpliSolveVariantCalling\n" << std::endl;
        std::cout << "Execution started under the following parameters:" << std::endl;
        std::cout << "\t1. Error estimation                               : " << a.error_file << std::endl;
        std::cout << "\t2. Tumour count dir                               : " << a.tumour_dir << std::endl;
        std::cout << "\t3. Output dir                                     : " << a.output_dir << std::endl;
        if (cov <= 0) {
            cov = 100;
            std::cout << "\t4. Coverage cutoff                                  : User gave: " << a.coverage_cutoff << ". The value is converted to default 100" << std::endl;
        } else {
            std::cout << "\t4. Coverage cutoff                                : " << cov << std::endl;
        }
        if (p_value <= 0 || p_value > 1) {
            p_value = 0.05f;
            std::cout << "\t5. p-value                                         : User gave: " << a.p_value << ". The value is converted to default 0.05" << std::endl;
        } else {
            std::cout << "\t5. p-value                                        : " << p_value << std::endl;
        }
        std::cout << std::endl;

        const Sharding shard(a.shard, a.native, a.output_dir);
        const ampli_host_shard *const sh = shard.sh;
        const bool writer = shard.writer(); // shard 0 writes the shared files of a multi-process run
        DevAsync dev_async;
        dev_async.start(); // beside the reading of the error table
        const std::string interm = a.output_dir + "/AmpliSolveVariantCalling_interm_files"; // VC:307
        mkdir_p(writer ? interm : a.output_dir);
        const double t0 = now_s();
        Panel panel;
        std::vector<float> thr;
        Background ring_teardown; // after the panel: joined before it goes away
        {
            PhaseClock::Scope sc("read_table");
            panel_from_error_table(a.error_file, writer ? interm + "/dummyVCF_1.vcf" : std::string(), panel, thr); // VC:320
        }
        std::cout << "Running function storeInputFile: the error levels have stored with success " << panel.walk.size() << std::endl;
        srand((unsigned)time(nullptr));
        const int seed = rand() % 1000;
        const std::string list_name = interm + "/" + std::to_string(seed) + "_tumour_count_list_original.txt"; // VC:332
        std::vector<std::pair<std::string, std::string>> files;
        {
            PhaseClock::Scope sc("list_files");
            files = list_count_files(a.tumour_dir, writer ? list_name : std::string());
        }
        const int total_samples = (int)files.size();
        int first_sample = 0;
        if (sh) files = shard_of_files(files, sh->index, sh->count, &first_sample);
        const int T = (int)files.size();
        std::cout << "\nRunning function storeList: " << list_name << " stored with success. It contains " << total_samples << " samples" << std::endl;
        if (sh) std::cout << "\tshard " << sh->index + 1 << "/" << sh->count << ": samples " << first_sample + 1 << ".." << first_sample + T << std::endl;
        std::cout << "\nRunning function callVariants...." << std::endl;

        const double t1 = now_s();
        const int64_t P = panel.P();
        std::vector<CallRow> rows;
        int64_t n_lines = 0;
        double parse_s = 0, rec_bytes_up = 0;
        int chunks_done = 0;
        if (T > 0 || !sh) { // a shard of a multi-process run may hold no tumour file
            // tumour files are independent given the error table: they stream through in chunks (parsing of the next
            // chunks overlaps upload + kernels of this one); only the emitted calls come back.  The parsers start before
            // the context is waited for.
            std::unique_ptr<ChunkStream> cs = open_stream(panel, files, true);
            Dev &dev = dev_async.get();
            float *d_thr = dev.upload(thr.data(), thr.size());
            uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());
            unsigned long long *d_n = alloc_call_counters(dev);
            DevSlot dslots[kDevSlots];
            for (Chunk *c; (c = next_chunk(*cs)) != nullptr;) {
                for (int64_t i = 0; i < c->n_irregular; ++i) std::cout << "malakia paizei edo" << std::endl; // VC:762-765
                const ampli_records r = upload_chunk(dev, dslots[c->slot % kDevSlots], *c, true);
                const int64_t R = P + c->E;
                uint8_t *d_mask = (uint8_t *)dslots[c->slot % kDevSlots].mask.ensure(dev, (size_t)c->n * R + 4);
                const char *why = collect_calls<ampli_call>(
                    dev, c->n, R, d_n,
                    [&](ampli_call *d_calls, int64_t cap, int attempt) {
                        PhaseClock::Scope sc(chunks_done == 0 && attempt == 0 ? "first_launch" : "launch"); // the first one loads the code object
                        clear_call_counters(dev, d_n);
                        dev.check(dev.api->poisson_call_records(dev.ctx, &r, P, d_thr, d_ref, cov, AMPLI_POISSON_PREFILTER, d_mask, d_calls, cap, d_n,
                                                                nullptr, nullptr), "ampli_poisson_call_records");
                    },
                    [] {}, [&](const ampli_call &cl) { rows.push_back(CallRow{call_base(*c, cl), cl.q_fw, cl.q_bw, cl.flags}); });
                if (why) throw Error{AMPLI_E_CAPACITY, std::string("variant calling did not complete a pass: ") + why};
                n_lines += c->n_lines;
                rec_bytes_up += (double)c->n * (double)(P + c->E) * (double)record_bytes(c->layout);
                ++chunks_done;
                cs->release(c);
            }
            parse_s = retire_stream(std::move(cs), a.process_ends, ring_teardown);
        }
        const double t2 = now_s();
        // Every emitted pair is scored once more here, with the reference's own operation sequence (score_reference_sequence:
        // kf_gammaq in double with the host's libm, the final log10 in x87 long double, VC:3834-3884), before it is gated,
        // flagged or printed: the device forms Q in fp64 with ROCm's exp / log and agrees to ~1e-10, which decides every pair
        // that is not within 1e-6 of the call gate Q >= 5 (VC:898; those are flagged by the kernel and listed either way) or of
        // the LowQ threshold Q < 20 (VC:1023) -- and since round 5 the PRINTED digits are the host's too, so that no column of
        // the Summary or the VCFs depends on the device's libm.  Sparse (0.1 % of the records), a few threads.
        int64_t n_guarded = 0, n_dropped = 0, n_dropped_unflagged = 0;
        {
            PhaseClock::Scope sc("guard_and_sort");
            std::vector<long double> qf(rows.size()), qb(rows.size());
            parallel_rows(rows.size(), 256, [&](size_t i, size_t i1) {
                for (; i < i1; ++i) {
                    const CallRow &c = rows[i];
                    qf[i] = score_reference_sequence(c.k_fw, c.rd - c.bw, thr[(size_t)(0 * 4 + c.alt) * P + c.p]); // VC:895
                    qb[i] = score_reference_sequence(c.k_bw, c.bw, thr[(size_t)(1 * 4 + c.alt) * P + c.p]);        // VC:896
                }
            });
            std::vector<CallRow> kept;
            kept.reserve(rows.size());
            for (size_t i = 0; i < rows.size(); ++i) {
                CallRow &c = rows[i];
                auto near = [](double q, double gate) { return std::fabs(q - gate) <= AMPLI_CALL_GATE_EPS; };
                const bool flagged = (c.flags & AMPLI_CALL_BORDERLINE) || near(c.q_fw, 20) || near(c.q_bw, 20);
                n_guarded += flagged ? 1 : 0;
                if (!(qf[i] >= 5 && qb[i] >= 5)) { // VC:898 in the reference's own arithmetic
                    ++n_dropped;
                    n_dropped_unflagged += flagged ? 0 : 1; // would mean device and host differ by more than the guard's 1e-6: reported below
                    continue;
                }
                c.q_fw = (double)qf[i];
                c.q_bw = (double)qb[i];
                kept.push_back(c);
            }
            if (n_dropped_unflagged)
                std::cerr << "warning: " << n_dropped_unflagged << " pair(s) passed the device's gate by more than 1e-6 and fail the host's; the host's arithmetic decides" << std::endl;
            rows.swap(kept);
            std::sort(rows.begin(), rows.end(), EmissionOrder{});
        }

        const std::string summary = a.output_dir + "/Summary_Variant_Info.txt"; // VC:342
        // multi-process run: every shard writes its rows to a part file; shard 0 concatenates them in shard order, which is
        // the visit order.  VC:1066 switches the stream to 4 significant digits inside the first row EVER written, so a
        // shard that is not the first to emit starts in that state.
        int64_t before = 0;
        if (sh) shard.hook(sh->rows_before(sh->user, (int64_t)rows.size(), &before), "rows_before");
        std::ofstream output(sh ? summary + ".part" + std::to_string(sh->index) : summary);
        if (before > 0) output << std::setprecision(4);
        if (writer)
        output << "Filename\tChrom\tPosition\tSubtitution\tRD\tRD_fw\tRD_bw\tAF\tReads_fw\tReads_bw\tAF_fw\tAF_bw\tAmpliconEdge_StrandBias\tFisherPvalue\tQscore_fw\tQscore_bw\tReadTier\tGermlineInfo\tMaxGermlineAF\t10merDownstream\t10merUpstream\tHomopolymerFlag" << std::endl; // VC:669
        // Annotation of the emitted calls (Fisher, context, flags: VC:902-1034) and the two text rows of each are independent
        // of every other call: formatted by a few threads, written in order.  VC:1066 sets std::setprecision(4) mid-row and it
        // sticks, so only the first row EVER written (this shard's row 0 when no shard before it emitted) prints its AF columns
        // with the stream's default 6 digits; every VCF row comes from a stream that is still at its default (VC:679).
        std::vector<std::string> sum_line(rows.size()), vcf_line(rows.size());
        {
            PhaseClock::Scope sc("annotate");
            // AMPLISOLVE_FISHER=off (validation only): leave the statement of VC:902 out, so that p keeps the -1 of VC:901 -- what the
            // reference's own callVariants does when it is compiled without its Fisher statements on a box without Boost
            // (oracle/Makefile, VC_CALL_DROP).  With it every byte of the Summary and the VCF bodies can be compared with that build.
            const char *fisher_env = getenv("AMPLISOLVE_FISHER");
            const bool fisher_off = fisher_env && std::string(fisher_env) == "off";
            parallel_rows(rows.size(), 64, [&](size_t i, size_t i1) {
                for (; i < i1; ++i)
                    std::tie(sum_line[i], vcf_line[i]) = annotate_row(rows[i], panel, files[(size_t)rows[i].sample].second, p_value, fisher_off, i == 0 && before == 0);
            });
        }
        PhaseClock::Scope sc_w("write_calls");
        size_t ri = 0;
        for (int t = 0; t < T; ++t) {
            const std::string &sample_name = files[(size_t)t].second;
            std::ofstream vcf(a.output_dir + "/" + sample_name + ".vcf"); // VC:679
            time_t now = time(0);
            char *dt = ctime(&now);
            vcf << "##fileformat=VCF-like\n##fileDate=" << dt
                << "##source=AmpliSolveVariantCalling\n##reference=Not_Specified_here\n##phasing=Not_Specified_here\n##FILTER=<ID=XXXXXXXXX,Description='XXXXXXXXX'>\n##FILTER=<ID=XXXXXXXXX,Description='XXXXXXXXX'>\n##FILTER=<ID=XXXXXXXXX,Description='XXXXXXXXX'>\n##FILTER=<ID=XXXXXXXXX,Description='XXXXXXXXX'>\n##INFO=<ID=RD,Number=1,Type=Integer,Description='Total Read Depth'>\n##SAMPLE=<ID=Not_Specified_here,SampleName="
                << sample_name
                << ">\n##INFO=<ID=AF,Number=.,Type=Float,Description='Allele Frequency'>\n##INFO=<ID=SR,Number=1,Type=String,Description='Supporting Reads'>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
                << std::endl; // VC:688
            if ((t + 1) % 50 == 0) std::cout << "\tParsed successfully " << t + 1 << "/" << T << "  samples" << std::endl;
            for (; ri < rows.size() && rows[ri].sample == t; ++ri) {
                vcf << vcf_line[ri];
                output << sum_line[ri];
            }
        }
        output.close();
        if (sh) {
            shard.hook(sh->barrier(sh->user), "barrier");
            if (writer) {
                std::ofstream all(summary, std::ios::binary);
                for (int k = 0; k < sh->count; ++k) {
                    const std::string part = summary + ".part" + std::to_string(k);
                    std::ifstream in(part, std::ios::binary);
                    if (!in) throw Error{AMPLI_E_INVALID, "missing Summary part of shard " + std::to_string(k) + " (is output_dir shared by all processes?)"};
                    // an empty part (a shard without calls that is not the header's writer) must not touch `all`:
                    // operator<<(streambuf*) sets failbit when it inserts nothing and every later part would be lost
                    if (in.peek() != std::ifstream::traits_type::eof()) all << in.rdbuf();
                    in.close();
                    if (!all.good()) throw Error{AMPLI_E_INVALID, "could not assemble " + summary + " from the shards' parts"};
                    std::remove(part.c_str());
                }
                all.close();
                if (all.fail()) throw Error{AMPLI_E_INVALID, "could not write " + summary};
            }
        }
        ring_teardown.wait();
        if (getenv("AMPLISOLVE_TIMING"))
            std::cerr << "TIMING table " << t1 - t0 << "\nTIMING stream " << t2 - t1 << " lines " << n_lines << " chunks " << chunks_done << " parse_busy "
                      << parse_s << " record_MB " << rec_bytes_up / 1e6 << " calls " << rows.size() << " guarded " << n_guarded << " dropped_by_guard " << n_dropped << "\nTIMING annotate+write " << now_s() - t2 << std::endl;
        std::cout << "\nAmpliSolveVariantCalling execution was successful. The results can be found at : " << summary << std::endl;
        std::cout << "\n" << kLine << std::endl;
        return 0;
    } catch (const Error &e) {
        return fail_banner(e);
    }
}

} // namespace ampli
