// amplisolve_amd/csrc/host/run_ee.cpp -- run_error_estimation re-states main() of AmpliSolveErrorEstimation.cpp (EE:241-520)
#include "pipeline.hpp"

namespace ampli {

int run_error_estimation(const EeArgs &a)
{
    try {
        // EE:328-388: numeric conversion and defaults
        float C_value = (float)std::atof(a.C_value.c_str());
        int cov = std::atoi(a.coverage_cutoff.c_str());
        const bool no_germlines = a.germline_dir == "not_available";
        float default_error = 0.01f;
        std::cout << kLine << "\n" << std::endl;
        std::cout << "                                Error estimation required for AmpliSolveVariantCalling program \n" << std::endl;
        std::cout << "                        MI355X-native build (amplisolve_amd); command line and files as AmpliSolveErrorEstimation\n" << std::endl;
        std::cout << "Execution started under the following parameters:" << std::endl;
        std::cout << "\t1. Panel design                                   : " << a.panel_design << std::endl;
        std::cout << "\t2. Reference genome                               : " << a.reference_genome << std::endl;
        if (no_germlines) {
            default_error = (float)std::atof(a.default_error.c_str());
            if (default_error > 0) {
                std::cout << "\t3. Germline count dir                             : NO germline count files available. Estimation of error is based on platform-specific error level given by user equal to " << default_error << std::endl;
            } else {
                default_error = 0.01f;
                std::cout << "\t3. Germline count dir                             : NO germline count files available. User gave wrong platform-specific error level and the estimation will be based on Error=" << default_error << std::endl;
            }
        } else {
            std::cout << "\t3. Germline count dir                             : " << a.germline_dir << std::endl;
        }
        if (C_value <= 0) {
            C_value = 0.002f;
            std::cout << "\t4. C value                                         : User gave: " << a.C_value << ". The value is converted to 0.002" << std::endl;
        } else {
            std::cout << "\t4. C value                                        : " << C_value << std::endl;
        }
        if (cov <= 0) {
            cov = 100;
            std::cout << "\t5. Coverage cutoff                                  : User gave: " << a.coverage_cutoff << ". The value is converted 100" << std::endl;
        } else {
            std::cout << "\t5. Coverage cutoff                                : " << cov << std::endl;
        }
        std::cout << "\t6. Output dir                                     : " << a.output_dir << std::endl;

        const Sharding shard(a.shard, a.native, a.output_dir);
        const ampli_host_shard *const sh = shard.sh;
        const bool writer = shard.writer(); // shard 0 writes every file of a multi-process run
        DevAsync dev_async;
        if (!no_germlines) dev_async.start(); // after the native shard (it may pick the device), beside the panel parsing
        const std::string interm = a.output_dir + "/AmpliSolveErrorEstimation_interm_files"; // EE:414
        if (writer) mkdir_p(interm);
        srand((unsigned)time(nullptr));
        const int seed = rand() % 1000; // EE:581-584

        double t0 = now_s();
        Panel panel;
        Background interm_files, ring_teardown; // declared after the panel: they are joined before it goes away
        {
            PhaseClock::Scope sc("panel");
            panel_from_bed(a.panel_design, panel);
            if (!a.refbases_file.empty()) panel_load_refbases_file(panel, a.refbases_file);
            else panel_load_fasta(panel, a.reference_genome);
            // the five by-product files of generateReferenceBases (EE:601-664) are read by nothing downstream
            if (writer) interm_files.run([&panel, interm, seed] {
                PhaseClock::Scope sc2("interm_files", false);
                panel_write_interm_files(panel, interm, seed);
            });
        }
        std::cout << "\nRunning function generateReferenceBases: Reference bases and amplicon duplicated positions have generated"
                  << "\n\t\t --> Parsed in total " << panel.rows.size() << " amplicons and annotated " << panel.walk.size() << " positions." << std::endl;
        std::cout << "Running function storeReference: panel reference bases stored with success " << panel.P() << std::endl;
        size_t ndup = 0;
        for (auto d : panel.dup) ndup += d;
        std::cout << "Running function storeDuplicates: panel duplicate positions stored with success " << ndup << std::endl;

        if (no_germlines) { // EE:472-506
            const std::string out = a.output_dir + "/positionSpecificNoise_default.txt";
            if (writer) write_error_table_default(panel, default_error, out);
            std::cout << "\nAmpliSolveErrorEstimation execution was successful. Results can be found at: " << out << std::endl;
            std::cout << "\n" << kLine << std::endl;
            return 0;
        }

        double t1 = now_s();
        const std::string list_name = interm + "/" + std::to_string(seed) + "_germline_count_list_original.txt"; // EE:442
        std::vector<std::pair<std::string, std::string>> files;
        {
            PhaseClock::Scope sc("list_files");
            files = list_count_files(a.germline_dir, writer ? list_name : std::string());
        }
        const int total_samples = (int)files.size();
        const std::vector<std::pair<std::string, std::string>> all_files = files; // the whole cohort in visit order (the in-order pass below)
        int first_sample = 0;
        if (sh) files = shard_of_files(files, sh->index, sh->count, &first_sample);
        const int S = (int)files.size();
        std::cout << "\nRunning function storeList: " << list_name << " stored with success. It contains " << total_samples << " samples" << std::endl;
        if (sh) std::cout << "\tshard " << sh->index + 1 << "/" << sh->count << ": samples " << first_sample + 1 << ".." << first_sample + S << std::endl;
        std::cout << "Running function storeGermlineStatistics:" << std::endl;

        // the parsers start NOW, into plain memory, while the runtime is still coming up on the side thread
        std::unique_ptr<ChunkStream> first_stream = S > 0 ? open_stream(panel, files, false) : nullptr;
        // the host copies of the table are made (their pages touched) while the runtime is still starting, not in front of the download
        const int64_t P = panel.P();
        std::vector<float> rate((size_t)P * 8), germ((size_t)P * 4);
        std::vector<uint8_t> code((size_t)P * 4), gp((size_t)P * 4);
        Dev &dev = dev_async.get();
        float *d_rate = dev.alloc<float>((size_t)P * 8), *d_germ = dev.alloc<float>((size_t)P * 4);
        uint8_t *d_code = dev.alloc<uint8_t>((size_t)P * 4), *d_gp = dev.alloc<uint8_t>((size_t)P * 4);
        int32_t *d_flags = dev.alloc<int32_t>(1);
        dev.check(dev.api->memset_d(dev.ctx, d_flags, 0, sizeof(int32_t)), "memset");
        // The accumulator table the chunks of a streamed cohort are folded into (EE:1057-1481 + the record loop of EE:1484-2544) is
        // streaming state and nothing else here (AMPLI_REDUCE_SUMMARY), so the compact-state kernel may carry it from chunk to chunk;
        // a cohort that arrives as ONE chunk needs no table at all: its launch finalises (one device) or stores slice-major (a shard).
        ampli_acc_table acc{};
        bool have_acc = false;
        auto need_acc = [&] {
            if (have_acc) return;
            void *d_accbuf = dev.alloc<char>(dev.api->acc_bytes(P));
            dev.check(dev.api->acc_bind(d_accbuf, P, &acc), "ampli_acc_bind");
            have_acc = true;
        };
        // a shard's exchange buffers are wanted by its LAST chunk's launch, which writes them (slice-major sums + germ-max pairs)
        void *xbufs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (sh) {
            shard.hook(sh->ee_buffers(sh->user, P, xbufs), "ee_buffers");
            for (void *b : xbufs)
                if (!b) throw Error{AMPLI_E_INVALID, "shard hook ee_buffers returned a null buffer"};
        }
        int launches_compact = 0, launches_compact24 = 0, launches_general = 0;
        void *ev = nullptr;
        dev.check(dev.api->event_create(&ev), "ampli_event_create");
        struct EvGuard { const HipApi *api; void *ev; ~EvGuard() { if (ev) api->event_destroy(ev); } } evg{dev.api, ev};
        DevSlot dslots[kDevSlots];
        int64_t n_lines = 0;
        double parse_s = 0, wait_s = 0, rec_bytes_up = 0;
        int chunks_done = 0;
        // The cohort streams through in chunks of samples: while chunk k is uploaded and reduced into the table, the
        // parser threads are already packing chunks k+1, k+2 into the other pinned buffers.  A depth beyond the fast
        // kernel's integer envelope is only known afterwards (a flag): the cohort then streams a second time through
        // the literal kernel.
        for (int attempt = 0; attempt < 2; ++attempt) {
            chunks_done = 0;
            n_lines = 0;
            rec_bytes_up = 0;
            if (S > 0) {
                std::unique_ptr<ChunkStream> cs = attempt == 0 ? std::move(first_stream) : open_stream(panel, files, false);
                for (Chunk *c; (c = next_chunk(*cs)) != nullptr;) {
                    if (attempt == 0) // the reference's own message, once per offending line (EE:1178-1181)
                        for (int64_t i = 0; i < c->n_irregular; ++i) std::cout << "malakia paizei edo" << std::endl;
                    const ampli_records r = upload_chunk(dev, dslots[c->slot % kDevSlots], *c, false);
                    const bool fuse = c->last && !sh; // one device holds the whole panel: finalize in the last chunk's launch
                    const bool only = c->last && chunks_done == 0; // the whole cohort (of this shard) in one chunk: no table
                    if (!only) need_acc();
                    const int32_t how = (chunks_done > 0 ? AMPLI_REDUCE_ACCUMULATE : 0) | AMPLI_REDUCE_SUMMARY;
                    {
                        PhaseClock::Scope sc(chunks_done == 0 && attempt == 0 ? "first_launch" : "launch"); // the first one loads the code object
                        if (c->last && sh)
                            dev.check(dev.api->error_reduce_records_sliced(dev.ctx, &r, P, first_sample + c->first, C_value, cov, only ? nullptr : &acc, how,
                                                                           sh->count, (double *)xbufs[0], (float *)xbufs[1]), "ampli_error_reduce_records_sliced");
                        else
                            dev.check(dev.api->error_reduce_records(dev.ctx, &r, P, first_sample + c->first, C_value, cov, only ? nullptr : &acc, how,
                                                                    fuse ? d_rate : nullptr, fuse ? d_code : nullptr, nullptr, fuse ? d_germ : nullptr,
                                                                    fuse ? d_gp : nullptr, fuse ? d_flags : nullptr), "ampli_error_reduce_records");
                        dev.check(dev.api->event_record(dev.ctx, ev), "ampli_event_record");
                        const int which = dev.api->last_reduce_kernel(dev.ctx); // 1 / 2: the compact-state kernel for uint16 / 24-bit records
                        (which == 1 ? launches_compact : which == 2 ? launches_compact24 : launches_general) += 1;
                    }
                    const double w0 = now_s();
                    {
                        PhaseClock::Scope sc("device_wait");
                        dev.check(dev.api->event_sync(ev), "ampli_event_sync"); // the chunk's buffers are free again
                    }
                    wait_s += now_s() - w0;
                    n_lines += c->n_lines;
                    rec_bytes_up += (double)c->n * (double)(P + c->E) * (double)record_bytes(c->layout);
                    ++chunks_done;
                    if ((first_sample + c->first + c->n) / 50 > (first_sample + c->first) / 50)
                        std::cout << "\tParsed successfully " << c->first + c->n << "/" << S << "  samples" << std::endl; // EE:1475-1478
                    cs->release(c);
                }
                parse_s += retire_stream(std::move(cs), a.process_ends, ring_teardown);
            }
            int32_t kflags = dev.flags();
            if (sh) shard.hook(sh->or_flags(sh->user, &kflags), "or_flags");
            if (!(kflags & AMPLI_FLAG_RERUN_GENERAL) || attempt == 1) break;
            dev.check(dev.api->set_tuning(dev.ctx, 0, 1, 0), "ampli_set_tuning"); // a depth beyond the fast kernel (on some shard): all stream again
            dev.check(dev.api->memset_d(dev.ctx, d_flags, 0, sizeof(int32_t)), "memset");
        }
        double t2 = now_s();
        std::cout << "Running function estimateThresholds: ";
        if (sh) {
            // multi-process run: this shard's table -> position-sliced exchange -> finalize of the own slice -> all-gather
            // -> plane-major table on every shard (include/amplisolve_hip.h, "Position-sliced merge")
            const int n = sh->count;
            const int64_t L = dev.api->slice_len(P, n);
            void **bufs = xbufs;
            if (chunks_done == 0) { // a shard without samples: zero sums, "no qualifying record" germ-max pairs (else: written by the last chunk's launch)
                std::vector<float> none((size_t)n * 8 * L);
                for (int k = 0; k < n; ++k)
                    for (int j = 0; j < 8; ++j)
                        std::fill_n(none.begin() + ((size_t)k * 8 + j) * L, (size_t)L, j < 4 ? -1.0f : -INFINITY);
                dev.check(dev.api->memset_d(dev.ctx, bufs[0], 0, (size_t)n * 21 * L * sizeof(double)), "memset");
                dev.check(dev.api->copy_h2d(dev.ctx, bufs[1], none.data(), none.size() * sizeof(float)), "ampli_copy_h2d");
                dev.sync();
            }
            shard.hook(sh->ee_exchange(sh->user), "ee_exchange");
            dev.check(dev.api->error_finalize_slice(dev.ctx, P, n, sh->index, (const double *)bufs[2], (const float *)bufs[3], C_value, cov,
                                                    bufs[4]), "ampli_error_finalize_slice");
            shard.hook(sh->ee_gather(sh->user), "ee_gather");
            dev.check(dev.api->error_table_unslice(dev.ctx, P, n, bufs[5], d_rate, d_code, nullptr, d_germ, d_gp, d_flags),
                      "ampli_error_table_unslice");
        } else if (chunks_done == 0) {
            throw Error{AMPLI_E_INVALID, "no sample could be read from " + a.germline_dir};
        }
        auto download_table = [&] {
            dev.download(rate.data(), d_rate, rate.size());
            dev.download(code.data(), d_code, code.size());
            dev.download(germ.data(), d_germ, germ.size());
            dev.download(gp.data(), d_gp, gp.size());
        };
        int32_t flags = 0;
        download_table();
        dev.download(&flags, d_flags, 1);
        dev.sync();
        if (flags & 1) {
            // A threshold sum left the exactness envelope (a coverage cut-off of a few reads with depths in the millions): its
            // double is no longer independent of the order of addition, and the reference always writes a table (EE:1597-1606, 1679-1704).
            // So the sums are formed once more in the reference's OWN order -- estimateThresholds' walk of `equal_range`, which libstdc++
            // hands out in reverse insertion order: the last file first, a position's later lines before its first -- one lane per position
            // (ampli_error_sums_inorder).  Every chunk of the WHOLE cohort stays resident for it (the walk starts at the last chunk); the
            // order-free planes (depth sums, counts, Germ_Max) come from an ordinary pass of the literal kernel over the same chunks.  Only
            // the process that writes the table does this (a shard's own table was merged in another order; nobody reads it again).
            std::cout << "\n\ta threshold sum is beyond the range in which its order of addition cannot matter: summing again in the reference's order" << std::endl;
            if (writer) {
                PhaseClock::Scope sc("inorder_pass");
                dev.check(dev.api->set_tuning(dev.ctx, 0, 1, 0), "ampli_set_tuning"); // the literal kernel: every plane exact, any depth
                need_acc();
                const std::unique_ptr<ChunkStream> cs = open_stream(panel, all_files, false);
                std::vector<std::unique_ptr<DevSlot>> resident;
                std::vector<ampli_records> descr;
                for (Chunk *c; (c = cs->next()) != nullptr;) {
                    resident.emplace_back(new DevSlot());
                    const ampli_records r = upload_chunk(dev, *resident.back(), *c, false);
                    dev.check(dev.api->error_reduce_records(dev.ctx, &r, P, c->first, C_value, cov, &acc, descr.empty() ? 0 : AMPLI_REDUCE_ACCUMULATE, nullptr, nullptr,
                                                            nullptr, nullptr, nullptr, nullptr), "ampli_error_reduce_records");
                    dev.sync(); // the chunk's host buffer is free again; its device copy stays
                    descr.push_back(r);
                    cs->release(c);
                }
                if (descr.empty()) throw Error{AMPLI_E_INVALID, "no sample could be read from " + a.germline_dir};
                for (size_t k = descr.size(); k-- > 0;)
                    dev.check(dev.api->error_sums_inorder(dev.ctx, &descr[k], P, C_value, cov, &acc, k + 1 == descr.size() ? 0 : 1), "ampli_error_sums_inorder");
                dev.check(dev.api->error_finalize(dev.ctx, &acc, C_value, cov, d_rate, d_code, nullptr, d_germ, d_gp, nullptr), "ampli_error_finalize");
                download_table();
                const int32_t kf = dev.flags();
                if (kf != 0) throw Error{AMPLI_E_HIP, "the in-order pass raised kernel flags " + std::to_string(kf)};
            }
        }
        double t3 = now_s();

        char name[64];
        snprintf(name, sizeof name, "positionSpecificNoise_%.4f.txt", (double)C_value); // EE:2556
        const std::string out = a.output_dir + "/" + name;
        if (writer) {
            PhaseClock::Scope sc("write_table");
            write_error_table(panel, rate.data(), code.data(), germ.data(), gp.data(), out);
        }
        {
            PhaseClock::Scope sc("join_background");
            interm_files.wait();
            ring_teardown.wait();
        }
        if (sh) shard.hook(sh->barrier(sh->user), "barrier");
        double t4 = now_s();
        std::cout << "\nAmpliSolveErrorEstimation execution was successful. Results can be found at: " << out << std::endl;
        if (getenv("AMPLISOLVE_TIMING"))
            std::cerr << "TIMING panel " << t1 - t0 << "\nTIMING stream " << t2 - t1 << " lines " << n_lines << " chunks " << chunks_done
                      << " parse_busy " << parse_s << " device_wait " << wait_s << " record_MB " << rec_bytes_up / 1e6 << "\nTIMING finish " << t3 - t2 << "\nTIMING write " << t4 - t3
                      // which error_reduce kernel each chunk's launch was (ampli_last_reduce_kernel): error_reduce_u16_kernel / error_reduce_u24_kernel
                      // (compact state) / error_reduce_kernel
                      << "\nTIMING reduce_launches " << launches_compact + launches_compact24 + launches_general << " error_reduce_u16_kernel " << launches_compact
                      << " error_reduce_u24_kernel " << launches_compact24 << " error_reduce_kernel " << launches_general
                      << " accumulator_table " << (have_acc ? 1 : 0) << std::endl;
        std::cout << "\n" << kLine << std::endl;
        return 0;
    } catch (const Error &e) {
        return fail_banner(e);
    }
}

} // namespace ampli
