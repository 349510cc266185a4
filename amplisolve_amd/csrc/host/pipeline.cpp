// amplisolve_amd/csrc/host/pipeline.cpp -- what the four command lines share (declared in pipeline.hpp): the phase clock, the device
// context and its buffers, the settings, the chunk stream's upload and retirement, the multi-GPU shard, the failure reports.
// The commands themselves: run_ee.cpp, run_vc.cpp (the two drop-in command lines), run_loo.cpp, run_dl.cpp.
// Parsing / formatting happen on the host; sums, rates, p-values and the call gate come from libamplisolve_hip.so.
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <chrono>
#include <mutex>

#include "pipeline.hpp"

namespace ampli {

// ---- PhaseClock ----
namespace {
struct PhaseEntry { std::string name; double s; bool critical; };
std::mutex g_phase_mu;
std::vector<PhaseEntry> g_phases;
} // namespace
double PhaseClock::now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
void PhaseClock::add(const char *name, double seconds, bool critical)
{
    std::lock_guard<std::mutex> lk(g_phase_mu);
    for (auto &e : g_phases)
        if (e.name == name && e.critical == critical) { e.s += seconds; return; }
    g_phases.push_back(PhaseEntry{name, seconds, critical});
}
void PhaseClock::reset()
{
    std::lock_guard<std::mutex> lk(g_phase_mu);
    g_phases.clear();
}
void PhaseClock::report(std::ostream &os, double wall)
{
    std::lock_guard<std::mutex> lk(g_phase_mu);
    double sum = 0;
    for (auto &e : g_phases) {
        os << "TIMING2 " << e.name << " " << e.s << (e.critical ? " critical" : " overlapped") << "\n";
        if (e.critical) sum += e.s;
    }
    // the wall clock (CLOCK_REALTIME) at this report, for a parent that wants to split what lies outside main() into the time
    // before main was entered and the time after the report (process teardown)
    const double epoch = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    os << "TIMING2 unattributed " << wall - sum << " critical\nTIMING2 wall_in_main " << wall << " total\nTIMING2 epoch_at_report "
       << std::fixed << std::setprecision(6) << epoch << " total" << std::endl;
    os.unsetf(std::ios::fixed);
}

void mkdir_p(const std::string &path) // generateFolder: `mkdir -p` (EE:3079-3086)
{
    std::string cur;
    for (size_t i = 0; i <= path.size(); ++i) {
        if (i == path.size() || path[i] == '/') {
            if (!cur.empty()) mkdir(cur.c_str(), 0777);
        }
        if (i < path.size()) cur.push_back(path[i]);
    }
}

void Dev::open()
{
    std::string why;
    {
        PhaseClock::Scope sc("hip_library_load", !side); // dlopen of libamplisolve_hip.so: pulls in the HIP runtime, registers the code object
        api = hip_api(&why);
    }
    if (!api) throw Error{AMPLI_E_HIP, "libamplisolve_hip.so could not be loaded (" + why + "); there is no CPU fallback"};
    {
        PhaseClock::Scope sc("runtime_init", !side); // the first HIP call of the process: HSA / driver start-up
        if (api->device_count() <= 0) throw Error{AMPLI_E_HIP, "no MI355X visible; there is no CPU fallback"};
    }
    int dev = 0;
    if (const char *e = getenv("AMPLISOLVE_DEVICE")) dev = atoi(e);
    {
        PhaseClock::Scope sc("context_create", !side); // hipSetDevice + properties + the first hipMalloc / hipMemset
        check(api->ctx_create(dev, nullptr, &ctx), "ampli_ctx_create");
    }
    if (side) warm_copies();
}
// The first copy in each direction sets up the runtime's copy machinery (staging buffers, the DMA queues: ~8 ms each,
// tools/micro/init_probe.cpp).  On the side thread that cost hides behind the parsers; paid later it sits on the main
// thread's path, in front of the first upload and of the table download.
void Dev::warm_copies()
{
    PhaseClock::Scope sc("warm_copies", false);
    const size_t n = 1 << 16;
    void *d = nullptr, *pin = nullptr;
    if (api->dev_alloc(ctx, n, &d) != AMPLI_OK) return;
    std::vector<char> pageable(n, 1);
    if (api->pinned_alloc(n, &pin) == AMPLI_OK) { // the uploads come from pinned (registered) memory
        memset(pin, 1, n);
        (void)api->copy_h2d(ctx, d, pin, n);
        (void)api->copy_d2h(ctx, pin, d, n);
    }
    (void)api->copy_h2d(ctx, d, pageable.data(), n); // small host arrays and the results travel pageable
    (void)api->copy_d2h(ctx, pageable.data(), d, n);
    (void)api->sync(ctx);
    if (pin) (void)api->pinned_free(pin);
    (void)api->dev_free(ctx, d);
}

namespace {

size_t chunk_bytes_setting()
{
    // about this many bytes of records (in the narrowest layout) per chunk (AMPLISOLVE_CHUNK_MB); ring_slots_setting() chunks may be parsed ahead
    size_t mb = 128;
    if (const char *e = getenv("AMPLISOLVE_CHUNK_MB")) mb = (size_t)std::max(1, atoi(e));
    if (const char *e = getenv("AMPLISOLVE_CHUNK_BYTES")) return (size_t)std::max(1ll, atoll(e)); // tests: down to one sample per chunk
    return mb << 20;
}

// Host ring slots.  The consumer needs the device context before it can take a chunk, and the HIP runtime's start-up takes 0.06-0.25 s:
// with the four slots of rounds 2-4 the parsers of a many-chunk cohort filled them and then stood still until the context was up
// (config-4-sized cohort, 13 chunks: wall = start-up + the rest of the parsing instead of the larger of the two).  So the ring may
// hold up to AMPLISOLVE_RING_MB (default 2048) of records in the narrowest layout, at least 4 and at most 64 slots; a slot's memory
// is only touched when a chunk is packed into it, and a cohort of fewer chunks allocates fewer slots.  (The device side: kDevSlots.)
int ring_slots_setting(const size_t chunk_bytes)
{
    size_t mb = 2048;
    if (const char *e = getenv("AMPLISOLVE_RING_MB")) mb = (size_t)std::max(1, atoi(e));
    const size_t n = (mb << 20) / std::max<size_t>(1, chunk_bytes);
    return (int)std::min<size_t>(64, std::max<size_t>(4, n));
}

// AMPLISOLVE_PIN: how a ring buffer reaches the device.  "register" (default): the parsers fill plain page-aligned memory
// -- they start before the HIP runtime is up -- and the buffer is pinned (hipHostRegister, ~6 ms per 128 MB) the first
// time it is uploaded from; "none": never pinned, the runtime stages the copy.  (Round 3 allocated the ring with
// hipHostMalloc: 23 ms per 128 MB up front, after the context was up, and 15 ms per 128 MB to free -- tools/micro/init_probe.cpp.)
bool pin_late()
{
    static const bool v = [] {
        const char *e = getenv("AMPLISOLVE_PIN");
        return !(e && std::string(e) == "none");
    }();
    return v;
}

// AMPLISOLVE_THREADS, or `unset`: the parser workers of a stream (0: the stream's own choice) and the cap of parallel_rows
int threads_setting(int unset) { const char *e = getenv("AMPLISOLVE_THREADS"); return e ? atoi(e) : unset; }

} // namespace

// The ring is up to 512 MB of touched, pinned memory.  Freeing it on a background thread takes ~35 ms during which the address
// space is write-locked again and again: the table writer / the annotation threads beside it stall in their own page faults
// (write_table 8 -> 30 ms on config 3).  An executable that is about to _exit leaves the buffers to the exit instead
// (AMPLISOLVE_RING_TEARDOWN=background restores the freeing, for comparison).
double retire_stream(std::unique_ptr<ChunkStream> cs, bool process_ends, Background &teardown)
{
    const double parse_s = cs->parse_seconds();
    PhaseClock::add("parser_busy", parse_s, false);
    if (const char *e = getenv("AMPLISOLVE_RING_TEARDOWN")) process_ends = std::string(e) == "exit";
    ChunkStream *done_stream = cs.release();
    if (process_ends) {
        done_stream->abandon();
        delete done_stream;
    } else { // a library caller lives on: unpin + unmap the ring, beside the download and the table writer / the annotation and the writers
        teardown.run([done_stream] {
            PhaseClock::Scope sc2("stream_teardown", false);
            delete done_stream;
        });
    }
    return parse_s;
}

// upload one chunk into its ring slot and describe it for the kernels
ampli_records upload_chunk(Dev &dev, DevSlot &ds, Chunk &c, bool for_calling)
{
    if (pin_late()) c.pin(dev.ctx);
    const size_t rb = record_bytes(c.layout);
    const size_t pb = (size_t)c.n * (size_t)c.P * rb, eb = (size_t)c.n * (size_t)c.E * rb;
    void *d_prim = ds.prim.ensure(dev, pb);
    dev.h2d(d_prim, c.prim, pb);
    ampli_records r;
    memset(&r, 0, sizeof r);
    r.recs = d_prim;
    r.row_stride = c.P;
    r.layout = c.layout;
    r.n_samples = c.n;
    r.E = c.E;
    if (c.E > 0) {
        void *d_ext = ds.ext.ensure(dev, eb);
        dev.h2d(d_ext, c.ext, eb);
        r.ext = d_ext;
        r.ext_stride = c.E;
        const std::vector<uint32_t> &aux = for_calling ? c.ext_pos : c.dup_off;
        void *d_aux = ds.aux.ensure(dev, aux.size() * sizeof(uint32_t));
        dev.h2d(d_aux, aux.data(), aux.size() * sizeof(uint32_t));
        if (for_calling) r.ext_pos = (const uint32_t *)d_aux;
        else r.dup_off = (const uint32_t *)d_aux;
    }
    if (!c.irregular.empty()) {
        // lines whose RD column is not A+C+G+T (EE:1178-1181, VC:762-765): the column travels as an int32 plane beside the
        // records (AMPLI_ABSENT = regular line) and the kernels use it where the reference does (EE:1229, VC:814, VC:895)
        std::vector<int32_t> rd((size_t)c.n * c.P, AMPLI_ABSENT), rde((size_t)c.n * c.E, AMPLI_ABSENT);
        for (const Irregular &x : c.irregular) {
            if ((int64_t)x.record < c.P) rd[(size_t)x.sample * c.P + x.record] = x.rd;
            else rde[(size_t)x.sample * c.E + (x.record - c.P)] = x.rd;
        }
        void *d_rd = ds.rd.ensure(dev, rd.size() * sizeof(int32_t));
        dev.h2d(d_rd, rd.data(), rd.size() * sizeof(int32_t));
        r.rd = (const int32_t *)d_rd;
        if (c.E > 0) {
            void *d_rde = ds.rd_ext.ensure(dev, rde.size() * sizeof(int32_t));
            dev.h2d(d_rde, rde.data(), rde.size() * sizeof(int32_t));
            r.rd_ext = (const int32_t *)d_rde;
        }
        dev.sync(); // the host vectors go out of scope
    }
    return r;
}

// The multi-GPU mode of the executables themselves (one process per GPU, no Python): the exchange steps of
// ampli_host_shard over the HIP library's own RCCL transport (ampli_comm_*).  Owns a context on the device's default
// stream -- the stream the pipeline's kernels run on -- so every collective is ordered with the kernels around it.
struct NativeShard {
    Dev dev;
    ampli_comm *comm = nullptr;
    ampli_host_shard hooks;
    NativeDist nd;
    std::string err;
    bool active = false;

    NativeShard() { memset(&hooks, 0, sizeof hooks); }
    ~NativeShard()
    {
        if (comm) dev.api->comm_destroy(comm);
    }
    void describe(const NativeDist &d)
    {
        nd = d;
        active = d.world > 1 || getenv("AMPLISOLVE_FORCE_NATIVE_DIST") != nullptr; // forced: the RCCL path on a communicator of one
        hooks.index = d.rank; hooks.count = d.world; hooks.user = this;
        hooks.ee_buffers = &NativeShard::s_buffers; hooks.ee_exchange = &NativeShard::s_exchange; hooks.ee_gather = &NativeShard::s_gather;
        hooks.or_flags = &NativeShard::s_or_flags; hooks.rows_before = &NativeShard::s_rows_before; hooks.barrier = &NativeShard::s_barrier;
    }
    // every rank gets here before it parses anything, so the rendezvous does not wait for the slowest parser
    void open()
    {
        std::string why;
        const HipApi *api = hip_api(&why);
        if (!api) throw Error{AMPLI_E_HIP, "libamplisolve_hip.so could not be loaded (" + why + "); there is no CPU fallback"};
        if (!getenv("AMPLISOLVE_DEVICE")) { // one GPU per process: rank k takes device k (mod the visible ones)
            const int n = api->device_count();
            if (n <= 0) throw Error{AMPLI_E_HIP, "no MI355X visible; there is no CPU fallback"};
            setenv("AMPLISOLVE_DEVICE", std::to_string(nd.rank % n).c_str(), 1);
        }
        if (nd.id_file.empty()) throw Error{AMPLI_E_INVALID, "multi-GPU run: AMPLISOLVE_ID_FILE (a path every process can see) is not set"};
        dev.open();
        const int crc = dev.api->comm_create(dev.ctx, nd.rank, nd.world, nd.id_file.c_str(), nd.timeout_s, &comm);
        if (crc == AMPLI_E_COMM_TIMEOUT) {
            // a detached helper thread is still inside ncclCommInitRank on this device: unwinding through ~Dev (hipFree,
            // context teardown) or exit()'s static destructors beside it can hang or crash.  Say why and leave at once.
            std::cout << "\t\t\nSomething went wrong: ampli_comm_create: " << dev.api->last_error(dev.ctx)
                      << "\n                                        Sorry but Amplisolve cannot continue..." << std::endl;
            std::cout.flush();
            std::cerr.flush();
            fflush(nullptr);
            _exit(1);
        }
        dev.check(crc, "ampli_comm_create");
        dev.check(dev.api->comm_barrier(comm), "ampli_comm_barrier"); // every rank has read the id
        if (nd.rank == 0) std::remove(nd.id_file.c_str());
    }

    size_t sums_b = 0, gm_b = 0, block_b = 0;
    int64_t L = 0;
    void *bufs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

    template <class F> static int guarded(void *user, F &&f)
    {
        NativeShard *s = (NativeShard *)user;
        try {
            f(*s);
            return 0;
        } catch (const Error &e) {
            s->err = e.msg;
            return e.code ? e.code : -1;
        }
    }
    static int s_buffers(void *user, int64_t P, void **out)
    {
        return guarded(user, [&](NativeShard &s) {
            const int n = s.nd.world;
            s.L = s.dev.api->slice_len(P, n);
            s.dev.check(s.dev.api->slice_bytes(P, n, &s.sums_b, &s.gm_b, &s.block_b), "ampli_slice_bytes");
            const size_t sizes[6] = {s.sums_b, s.gm_b, s.sums_b / (size_t)n, s.gm_b, s.block_b, s.block_b * (size_t)n};
            for (int i = 0; i < 6; ++i) {
                s.bufs[i] = s.dev.alloc<char>(sizes[i]);
                s.dev.check(s.dev.api->memset_d(s.dev.ctx, s.bufs[i], 0, sizes[i]), "ampli_memset_d"); // padding positions are never written
                out[i] = s.bufs[i];
            }
        });
    }
    static int s_exchange(void *user)
    {
        return guarded(user, [&](NativeShard &s) {
            s.dev.check(s.dev.api->comm_reduce_scatter_f64(s.comm, (const double *)s.bufs[0], (double *)s.bufs[2], 21 * s.L), "ampli_comm_reduce_scatter_f64");
            s.dev.check(s.dev.api->comm_all_to_all_f32(s.comm, (const float *)s.bufs[1], (float *)s.bufs[3], 8 * s.L), "ampli_comm_all_to_all_f32");
        });
    }
    static int s_gather(void *user)
    {
        return guarded(user, [&](NativeShard &s) {
            s.dev.check(s.dev.api->comm_all_gather_bytes(s.comm, s.bufs[4], s.bufs[5], (int64_t)s.block_b), "ampli_comm_all_gather_bytes");
        });
    }
    static int s_or_flags(void *user, int32_t *flags)
    {
        return guarded(user, [&](NativeShard &s) {
            int32_t bits[31];
            for (int b = 0; b < 31; ++b) bits[b] = (*flags >> b) & 1;
            s.dev.check(s.dev.api->comm_all_reduce_max_i32(s.comm, bits, 31), "ampli_comm_all_reduce_max_i32");
            int32_t v = 0;
            for (int b = 0; b < 31; ++b) v |= bits[b] ? (1 << b) : 0;
            *flags = v;
        });
    }
    static int s_rows_before(void *user, int64_t mine, int64_t *before)
    {
        return guarded(user, [&](NativeShard &s) { s.dev.check(s.dev.api->comm_exclusive_sum_i64(s.comm, mine, before), "ampli_comm_exclusive_sum_i64"); });
    }
    static int s_barrier(void *user)
    {
        return guarded(user, [&](NativeShard &s) { s.dev.check(s.dev.api->comm_barrier(s.comm), "ampli_comm_barrier"); });
    }
};

Sharding::Sharding(const ampli_host_shard *given, const NativeDist &nd, const std::string &output_dir) : sh(given && given->count > 1 ? given : nullptr)
{
    if (sh) return;
    native.reset(new NativeShard); // the executables' own multi-GPU mode (RCCL); callers with their own transport pass `given`
    native->describe(nd);
    if (!native->active) return;
    mkdir_p(output_dir); // the default id file lives there
    native->open();
    sh = &native->hooks;
}
void Sharding::hook(int rc, const char *what) const
{
    if (rc != 0) throw Error{AMPLI_E_INVALID, std::string("shard hook failed: ") + what + (!native || native->err.empty() ? "" : " -- " + native->err)};
}

std::unique_ptr<ChunkStream> open_stream(const Panel &panel, const std::vector<std::pair<std::string, std::string>> &files, bool keep_line_no)
{
    const size_t chunk_bytes = chunk_bytes_setting();
    return std::unique_ptr<ChunkStream>(new ChunkStream(panel, files, threads_setting(0), keep_line_no, chunk_bytes, ring_slots_setting(chunk_bytes)));
}

int row_threads(size_t n, size_t grain)
{
    const int nt = (int)std::min<size_t>(std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency())), std::max<size_t>(1, n / grain));
    return std::max(1, std::min(nt, threads_setting(nt)));
}
void parallel_rows(size_t n, size_t grain, const std::function<void(size_t, size_t)> &fn)
{
    const int nt = row_threads(n, grain);
    auto part = [&](int tid) { fn(n * (size_t)tid / (size_t)nt, n * (size_t)(tid + 1) / (size_t)nt); };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(part, t);
    part(0);
    for (auto &t : th) t.join();
}

int fail_banner(const Error &e)
{
    std::cout << "\t\t\nSomething went wrong: " << e.msg << std::endl;
    std::cout << "                                        Sorry but Amplisolve cannot continue..." << std::endl;
    std::cout << kLine << std::endl;
    return e.code ? e.code : -1;
}

void finish_process(int status)
{
    const char *e = getenv("AMPLISOLVE_EXIT");
    if (e && std::string(e) == "orderly") return;
    std::cout.flush();
    std::cerr.flush();
    fflush(nullptr);
    _exit(status);
}

NativeDist native_dist_from_env(const std::string &output_dir)
{
    NativeDist d;
    if (const char *e = getenv("AMPLISOLVE_WORLD_SIZE")) d.world = std::max(1, atoi(e));
    if (const char *e = getenv("AMPLISOLVE_RANK")) d.rank = atoi(e);
    if (d.rank < 0 || d.rank >= d.world) { d.rank = 0; d.world = 1; }
    if (const char *e = getenv("AMPLISOLVE_ID_FILE")) d.id_file = e;
    else if (!output_dir.empty()) d.id_file = output_dir + "/.amplisolve_rccl_id"; // output_dir is shared by all processes anyway
    if (const char *e = getenv("AMPLISOLVE_RCCL_TIMEOUT")) d.timeout_s = std::max(1, atoi(e));
    return d;
}

} // namespace ampli
