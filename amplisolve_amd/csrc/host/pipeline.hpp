// amplisolve_amd/csrc/host/pipeline.hpp -- the device plumbing every command line shares: the context, the chunk stream, the call list.
// Internal to run_ee.cpp, run_vc.cpp, pipeline.cpp and command.hpp / command.cpp, through which the project's own nine commands
// (run_loo.cpp, run_dl.cpp, run_dp.cpp, run_pd.cpp, run_sc.cpp, run_ct.cpp, run_ac.cpp, run_ss.cpp, run_ex.cpp) take it together with
// what only they share.  All eleven commands and their arguments are declared in host.hpp; the *_main.cpp files need no more than
// that and main_args.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <memory>
#include <sstream>
#include <thread>

#include "hip_loader.hpp"
#include "host.hpp"

namespace ampli {

void mkdir_p(const std::string &path); // generateFolder: `mkdir -p` (EE:3079-3086)
inline double now_s() { return PhaseClock::now(); }
constexpr const char *kLine = "************************************************************************************************************************************";

struct Dev {
    const HipApi *api = nullptr;
    ampli_ctx *ctx = nullptr;
    std::vector<void *> allocs;
    ~Dev()
    {
        if (ctx) {
            PhaseClock::Scope sc("device_teardown");
            for (void *p : allocs) api->dev_free(ctx, p);
            api->ctx_destroy(ctx);
        }
    }
    void check(int rc, const char *what)
    {
        if (rc != AMPLI_OK)
            throw Error{rc, std::string(what) + ": " + api->strerror_(rc) + (ctx ? std::string(" -- ") + api->last_error(ctx) : "")};
    }
    bool side = false; // opened on a side thread: its start-up spans are overlapped work, not the main thread's path
    void open();
    void warm_copies();
    template <class T> T *alloc(size_t n)
    {
        PhaseClock::Scope sc("device_alloc");
        void *p = nullptr;
        check(api->dev_alloc(ctx, n * sizeof(T), &p), "ampli_dev_alloc");
        allocs.push_back(p);
        return (T *)p;
    }
    void free(void *p)
    {
        PhaseClock::Scope sc("device_alloc");
        for (auto it = allocs.begin(); it != allocs.end(); ++it)
            if (*it == p) { allocs.erase(it); break; }
        check(api->dev_free(ctx, p), "ampli_dev_free");
    }
    void h2d(void *d, const void *src, size_t bytes)
    {
        PhaseClock::Scope sc("h2d_enqueue");
        check(api->copy_h2d(ctx, d, src, bytes), "ampli_copy_h2d");
    }
    template <class T> T *upload(const T *src, size_t n)
    {
        T *d = alloc<T>(n ? n : 1);
        if (n) h2d(d, src, n * sizeof(T));
        return d;
    }
    template <class T> void download(T *dst, const T *d, size_t n)
    {
        PhaseClock::Scope sc("d2h");
        check(api->copy_d2h(ctx, dst, d, n * sizeof(T)), "ampli_copy_d2h");
    }
    void sync()
    {
        PhaseClock::Scope sc("device_wait");
        check(api->sync(ctx), "ampli_sync");
    }
    int32_t flags() // the AMPLI_FLAG_* bits the kernels raised so far, read and cleared
    {
        PhaseClock::Scope sc("device_wait");
        int32_t f = 0;
        check(api->ctx_flags(ctx, &f, 1), "ampli_ctx_flags");
        return f;
    }
};

// a device buffer that only ever grows (one per ring slot and kind)
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    void *ensure(Dev &dev, size_t bytes)
    {
        if (bytes > cap) {
            if (p) dev.free(p);
            p = nullptr;
            cap = bytes + bytes / 8 + 256;
            p = dev.alloc<char>(cap);
        }
        return p;
    }
};

struct DevSlot { DevBuf prim, ext, aux, mask, rd, rd_ext; };
// The device side keeps four buffers: a chunk is uploaded, consumed and waited for before the next one is taken, so ring slot k
// simply uses device buffer k mod 4 (the host ring may be longer: ring_slots_setting in pipeline.cpp).
constexpr int kDevSlots = 4;

// work that nothing downstream waits for (by-product files, freeing the ring): runs beside the main thread, joined when the
// owner leaves its scope; an exception is rethrown by wait()
struct Background {
    std::thread th;
    std::exception_ptr ex;
    template <class F> void run(F &&f)
    {
        wait();
        th = std::thread([this, f]() mutable {
            try {
                f();
            } catch (...) {
                ex = std::current_exception();
            }
        });
    }
    void wait()
    {
        if (th.joinable()) th.join();
        if (ex) {
            std::exception_ptr e = ex;
            ex = nullptr;
            std::rethrow_exception(e);
        }
    }
    ~Background()
    {
        if (th.joinable()) th.join();
    }
};

// The context is opened on a side thread while the main thread reads the panel / the error table: loading the HIP runtime and
// the code object takes 0.1-0.2 s, a good part of a command line's wall time on small and medium cohorts.
struct DevAsync {
    Dev dev;
    Background side; // after dev: joined before the context goes away
    bool started = false;
    void start()
    {
        started = true;
        dev.side = true;
        side.run([this] { dev.open(); });
    }
    Dev &get() // the opened context; rethrows what open() threw (no device, no library: there is no CPU fallback)
    {
        if (!started) start();
        PhaseClock::Scope sc("wait_for_context"); // what of the start-up the panel / table parsing did not hide
        side.wait();
        return dev;
    }
};

// the cohort's stream with the settings of AMPLISOLVE_THREADS, _CHUNK_MB / _CHUNK_BYTES and _RING_MB; the parsers start at once
std::unique_ptr<ChunkStream> open_stream(const Panel &panel, const std::vector<std::pair<std::string, std::string>> &files, bool keep_line_no);
inline Chunk *next_chunk(ChunkStream &cs) { PhaseClock::Scope sc("wait_for_parser"); return cs.next(); }
// a stream whose last chunk was released: leaves its ring to the exit or frees it on `teardown`; returns its parser seconds
double retire_stream(std::unique_ptr<ChunkStream> cs, bool process_ends, Background &teardown);
// upload one chunk into its ring slot and describe it for the kernels
ampli_records upload_chunk(Dev &dev, DevSlot &ds, Chunk &c, bool for_calling);

// Which shard of a multi-process run this process is: `given` when the caller brings its own transport (count > 1), else the
// executables' own multi-GPU mode over RCCL (NativeShard, pipeline.cpp) when `nd` asks for it, else none (sh == nullptr).
struct NativeShard;
struct Sharding {
    const ampli_host_shard *sh;
    std::shared_ptr<NativeShard> native; // (shared_ptr: NativeShard is a complete type in pipeline.cpp only)
    Sharding(const ampli_host_shard *given, const NativeDist &nd, const std::string &output_dir);
    bool writer() const { return !sh || sh->index == 0; } // shard 0 writes the shared files of a multi-process run
    void hook(int rc, const char *what) const;             // the status of a shard hook: throws Error unless 0
};

// fn(i0, i1) over [0, n) split evenly over row_threads(n, grain) threads
void parallel_rows(size_t n, size_t grain, const std::function<void(size_t, size_t)> &fn);

// what a failed command prints, and its exit status: the reference's banner (EE / VC) or one line (LOO / DL)
int fail_banner(const Error &e);
inline int fail_line(const char *program, const std::string &why) { std::cout << program << " failed: " << why << std::endl; return 1; }

// ---- the emitted calls ----
// Where a record of a chunk came from: the data line of its sample's file (-1: absent) and the panel position of record slot r in
// [0, P + E).  H is the Chunk, or a copy of these members that outlives it (leave-one-out's Resident).
template <class H> int record_line(const H &h, int s, int64_t r) { return r < h.P ? h.line_prim[(size_t)s * h.P + r] : h.line_ext[(size_t)s * h.E + (r - h.P)]; }
template <class H> int64_t record_position(const H &h, int64_t r) { return r < h.P ? r : (int64_t)h.ext_pos[(size_t)(r - h.P)]; }

struct CallBase {
    int sample, line, alt; // sample: index in this process's range of the visit order
    int64_t p;             // panel position
    float af, af_fw, af_bw;
    int rd, fw, bw, k_fw, k_bw; // the evidence of the call, as the kernel saw it
};
template <class H> CallBase call_base(const H &h, const ampli_call &cl)
{
    return CallBase{h.first + cl.sample, record_line(h, cl.sample, cl.record), cl.alt, record_position(h, cl.record), cl.af, cl.af_fw, cl.af_bw,
                    cl.rd, cl.fw, cl.bw, cl.k_fw, cl.k_bw};
}
// emission order: samples in visit order, lines in file order, alts in A,C,G,T order (VC:672, 723, 869-3283)
struct EmissionOrder {
    bool operator()(const CallBase &x, const CallBase &y) const
    {
        if (x.sample != y.sample) return x.sample < y.sample;
        if (x.line != y.line) return x.line < y.line;
        return x.alt < y.alt;
    }
};

// the counters of the sharded call list (d_n below), and their reset in front of a pass that does not reset them itself
inline unsigned long long *alloc_call_counters(Dev &dev) { return dev.alloc<unsigned long long>(AMPLI_CALL_COUNTER_WORDS); }
inline void clear_call_counters(Dev &dev, unsigned long long *d_n)
{
    dev.check(dev.api->memset_d(dev.ctx, d_n, 0, sizeof(unsigned long long) * AMPLI_CALL_COUNTER_WORDS), "memset");
}
// One pass of ampli_poisson_call_records / ampli_loo_call_records over n_samples x R records, repeated until its sharded call list
// (include/amplisolve_hip.h: AMPLI_CALL_SHARDS segments, one counter each in d_n) and the prefilter queue held everything:
// launch(d_calls, cap, attempt) issues the pass into a list of `cap` entries, undo() takes back what a pass that has to be repeated
// added outside the list, each(call) sees every call of the pass that fit.  Returns nullptr, or what overflowed in the last attempt.
template <class Call, class Launch, class Undo, class Each>
const char *collect_calls(Dev &dev, int64_t n_samples, int64_t R, unsigned long long *d_n, Launch launch, Undo undo, Each each)
{
    const char *why = nullptr;
    int64_t cap = std::max<int64_t>(1 << 16, n_samples * R / 16);
    for (int attempt = 0; attempt < 6; ++attempt) {
        cap -= cap % AMPLI_CALL_SHARDS;
        const int64_t per = cap / AMPLI_CALL_SHARDS;
        Call *d_calls = dev.alloc<Call>((size_t)cap);
        launch(d_calls, cap, attempt);
        std::vector<unsigned long long> n(AMPLI_CALL_COUNTER_WORDS);
        why = nullptr;
        if (dev.flags() & AMPLI_FLAG_QUEUE_OVERFLOW) { // more survivors than the default queue holds: size it for the worst case
            dev.check(dev.api->set_queue_items(dev.ctx, n_samples * R * 3), "ampli_set_queue_items");
            why = "prefilter queue still overflowing";
        } else {
            dev.download(n.data(), d_n, n.size());
            dev.sync();
            unsigned long long worst = 0, total = 0;
            for (int k = 0; k < AMPLI_CALL_SHARDS; ++k) {
                worst = std::max(worst, n[(size_t)k * AMPLI_CALL_COUNTER_STRIDE]);
                total += n[(size_t)k * AMPLI_CALL_COUNTER_STRIDE];
            }
            if ((int64_t)worst > per) {
                // a segment overflowed.  Which segment a call lands in depends on the order the workgroups ran in, so
                // the rerun is sized with headroom: every segment could hold ALL calls of this pass, capped at the
                // number of (record, alt) pairs there are
                cap = (int64_t)std::min<unsigned long long>((unsigned long long)n_samples * R * 3, std::max(total, 2 * worst)) * AMPLI_CALL_SHARDS;
                why = "call list still overflowing";
            }
        }
        if (why) undo();
        for (int k = 0; k < AMPLI_CALL_SHARDS && !why; ++k) {
            const size_t cnt = (size_t)n[(size_t)k * AMPLI_CALL_COUNTER_STRIDE];
            std::vector<Call> calls(cnt);
            if (cnt) dev.download(calls.data(), d_calls + (size_t)k * per, cnt);
            dev.sync();
            for (const Call &cl : calls) each(cl);
        }
        dev.free(d_calls); // a repeated attempt gets a list of its own size
        if (!why) break;
    }
    return why;
}

} // namespace ampli
