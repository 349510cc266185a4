"""The stream contract of Context made testable -- TEST INFRASTRUCTURE.

Every device operation a Context method causes has to be ordered on the context's stream.  On one stream, or on two streams that share
a hardware queue, a misplaced fill, upload, readback or kernel is serialised with everything else and gives the right answer; on two
streams that overlap it gives the right answer almost always.  This module makes it give the WRONG answer, every time:

  * Env finds a torch.cuda.Stream S that overlaps the other stream (torch's default stream, or a created stream D where no candidate
    overlaps the default stream) in both directions, with the probe ampli_set_ranges uses (a delay on X, a tiny copy on Y, synchronise
    Y, X's event is not complete), and creates the Context under torch.cuda.stream(S) -- the documented embedding.
  * s_delayed(): the device inputs hold a decoy B and the outputs the sentinel of tests/helpers.py (0xFF; zeros where the contract says
    ADDED TO); S gets a delay, then the copies of the real inputs A and the sentinel again, then the method is called with torch's
    current stream the OTHER one, then the outputs are copied out on S.  Everything was enqueued while the delay ran (asserted), so
    whatever ran off S read B, or was overwritten by the sentinel, or read the sentinel.
  * other_delayed(): the delay sits on the other stream; the pools of both streams are primed with sentinel blocks; the method is called
    without outputs of the caller's and with host arrays where it takes them; after ctx.sync() the other stream's delay must still run
    and the results must be right, then and once more after the other stream has caught up: a zero fill, an upload or an allocation
    on the other stream is late, blocks the host, or lands on the results after the kernel.
A and B have identical shapes and differ only in values that cannot index memory (counts, bases, qualities, thresholds, weights), never
in offsets, CSR bounds, rec_off, CIGARs, lengths or keys: any mixture of them is a valid input, whatever is misplaced.

CASES lists one case per device-working Context method; tests/test_stream_order_complete.py holds the list against the class and
the header.  Expected values: the oracle / the host generator where they are callable at the shape (the core pass, synth_*), else the
same call on the session's default-stream context at a shape the method's own test holds to its model (the world of
tests/test_gpu_wide_offsets.py, the case tables of the read walks, tests/fdr_planes.py).  Bytes are compared exactly."""
import ctypes as C
import dataclasses
import functools
import inspect
import re
import time

import numpy as np

SENTINEL = 0xFF
MAX_DELAY_MS = 500.0
# Five times the longest host enqueue of any case below, measured on the finished tree from the launch of the delay to the check that it
# still runs: tumour_fraction with host lists in other_delayed(), 4.55 ms (three uploads from pageable memory, the kernel, the
# synchronisation); every other case takes under 1 ms
DELAY_MS = 23.0
PROBE_MS = 10.0
CANDIDATES = 8

# (where the line stands, the line): what lets a case skip the still-running assertion of s_delayed().  tests/test_stream_order_complete.py
# finds every line in its file (white space folded), so a case cannot outlive the sentence it rests on.
HEADER, API = "include/amplisolve_hip.h", "amplisolve_amd/api.py"
SYNC_FLAGS = (HEADER, "Flags raised by kernels of this context since the last clear (synchronises the stream).")
SYNC_LIMIT = (HEADER, "the most evaluations of one strand; reset != 0 clears them. Synchronises the stream.")
SYNC_POWER = (HEADER, "tail; reset != 0 clears them. Synchronises the stream.")
SYNC_MERGE = (HEADER, "Synchronises the stream: the list of the parts' pointers is uploaded from the caller's stack.")
SYNC_HOST = (API, "A method that returns host values (flags, pack16 / pack24's fits, read_calls, read_loo_calls, n_calls_total, the limit and power "
                  "statistics) synchronises that stream and no other.")

# (case, mode) -> host milliseconds from the launch of the delay to the check that it still runs: what the delay has to outlast.  (In
# s_delayed() a case that synchronises the stream waits for the delay itself: its figure is the delay, not an enqueue time.)
ENQUEUE_MS = {}


# ---------------------------------------------------------------------------------------------------------------------------
# small things
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    """a numpy array on the device, on torch's current stream"""
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _host(t):
    return t.detach().contiguous().cpu().numpy()


def _bytes(t):
    """a device tensor as a flat uint8 view (a copy where it is not contiguous: on torch's current stream)"""
    import torch

    return t.contiguous().view(-1).view(torch.uint8)


def _csr32(off, ent):
    """a host CSR as the int32 arrays (read as uint32) the device form of the argument is"""
    return np.asarray(off, np.int64).astype(np.uint32).view(np.int32), np.asarray(ent, np.int64).astype(np.uint32).view(np.int32)


def _table(fin):
    """the error table as results: germ_val is defined where germ_present is set only (post_table masks the rest on the host)"""
    return dict(rate=fin.rate, code=fin.code, thr=fin.thr, germ_val=fin.germ_val, germ_present=fin.germ_present, flags=fin.flags)


def post_table(h):
    if "germ_val" in h and "germ_present" in h:
        h = dict(h)
        gv = h["germ_val"].view(np.float32).copy()
        gv[h["germ_present"].view(np.uint8) == 0] = 0
        h["germ_val"] = gv.view(np.uint8)
    return h


def _table_outs(P):
    return dict(rate=((2, 4, P), np.float32, "over"), code=((4, P), np.uint8, "over"), thr=((2, 4, P), np.float32, "over"),
                germ_val=((4, P), np.float32, "over"), germ_present=((4, P), np.uint8, "over"), flags=((1,), np.int32, "add"))


def _given_table(o):
    from amplisolve_amd.api import ErrorTable

    return ErrorTable(**{k: o[k] for k in ("rate", "code", "thr", "germ_val", "germ_present", "flags")}) if "rate" in o else None


def _acc(ctx, P, buf):
    from amplisolve_amd.api import Acc

    return Acc(ctx, P, buf=buf)


def _acc_bytes(P):
    from amplisolve_amd import hip_lib

    return int(hip_lib().ampli_acc_bytes(P))


ACC_SUMS = ("snt", "srd", "cnt", "nrec")


def _planes(acc, names=ACC_SUMS + ("gm_n",)):
    return {k: getattr(acc, k) for k in names}


# ---------------------------------------------------------------------------------------------------------------------------
# the case
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    methods: tuple                 # the Context methods the case runs
    inputs: object                 # (world, "A" | "B") -> {name: numpy array}: what lies on the device (or is handed over as a host array)
    call: object                   # (ctx, x, o) -> {name: device tensor | host value}; x: the inputs, o: the outputs the caller brings
    outs: object = None            # (world) -> {name: (shape, numpy dtype, "over" | "add")}
    required: tuple = ()           # outputs the method cannot allocate itself: brought in both modes
    host_ok: tuple = ()            # inputs the method also takes as host arrays: handed over as such in other_delayed()
    setup: object = None           # (ctx): settings of the context, before anything is enqueued
    teardown: object = None
    syncs: tuple = None            # (file, line): the line that says the method synchronises the stream: no not-complete assertion in s_delayed()
    protos: tuple = ()             # C entry points the case calls beside those its methods name
    post: object = None            # host results -> host results (cells a contract leaves undefined)
    model: object = None           # (A's inputs) -> {name: numpy array}: expected values from a model, where one is callable
    same_ab: bool = False          # no inputs on the device: A and B cannot differ

    def entry_points(self):
        from amplisolve_amd import Context

        out = set(self.protos)
        todo, seen = list(self.methods), set()
        while todo:  # a method, and the private helpers and public methods it calls on self
            m = todo.pop()
            if m in seen or not hasattr(Context, m):
                continue
            seen.add(m)
            raw = vars(Context)[m]
            src = inspect.getsource(raw.fn if hasattr(raw, "fn") else inspect.unwrap(raw))
            out |= set(re.findall(r"self\.lib\.(ampli_\w+)", src))
            todo += re.findall(r"self\.(_\w+)\(", src)
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# the two streams, the delay, the context
# ---------------------------------------------------------------------------------------------------------------------------
class Env:
    def __init__(self):
        import torch

        from amplisolve_amd import Context

        self.torch = torch
        self.default = torch.cuda.default_stream()
        self.cycles_per_ms = self._calibrate()
        self.tiny_d = torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.tiny_h = torch.zeros(16, dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        self.tried, self.rejected = [], []
        self.S, self.other, self.other_is_default, self.ctx = None, None, True, None
        cands = [torch.cuda.Stream() for _ in range(CANDIDATES)]
        for name, other in (("default", self.default), ("D", None)):
            if other is None:  # no candidate serves with torch's default stream: a created stream D made torch's current stream
                other = torch.cuda.Stream()
            for s in cands:
                c = self._accept(name, other, s)
                if c is not None:
                    self.S, self.other, self.ctx, self.other_is_default = s, other, c, name == "default"
                    break
            if self.S is not None:
                break
        self.ctx_other = None
        if self.S is not None:
            with torch.cuda.stream(self.other):
                self.ctx_other = Context(0)  # the wrong wrappers' second context

    def _accept(self, name, other, s):
        """a Context on candidate s, if s overlaps the other stream both ways and so do the streams of the context's two position ranges
        (they are the library's own, dealt to the hardware queues like any other: one that shares a queue with the other stream would
        wait behind its delay whatever the method did).  A rejected context stays alive until the search ends: destroyed at once, the
        next one's streams would take its place on the same queues."""
        from amplisolve_amd import Context

        torch = self.torch
        if not (self.overlap(other, s) and self.overlap(s, other)):
            self.tried.append((name, hex(s.cuda_stream), False, None))
            return None
        with torch.cuda.stream(s):
            c = Context(0)
        c.set_ranges(2)
        lanes = all(self.lane_overlaps(other, c, k) for k in range(2))
        c.set_ranges(1)  # (the ranges' streams are kept for the next set_ranges(2))
        self.tried.append((name, hex(s.cuda_stream), True, lanes))
        if lanes:
            return c
        self.rejected.append(c)
        return None

    def lane_overlaps(self, other, c, k):
        """do two events on range k's stream complete while a delay runs on the other stream?"""
        torch = self.torch
        torch.cuda.synchronize()
        e0, e1 = c.event(), c.event()
        try:
            with torch.cuda.stream(other):
                torch.cuda._sleep(self.cycles(PROBE_MS))
                ev = torch.cuda.Event()
                ev.record(other)
            c.range_record(k, e0)
            c.range_record(k, e1)
            c.elapsed_ms(e0, e1)  # waits for e1
            running = not ev.query()
            torch.cuda.synchronize()
        finally:
            for e in (e0, e1):
                c.lib.ampli_event_destroy(e)
        return running

    def require(self):
        assert self.S is not None, (f"no pair of streams overlaps (delay on X, copy on Y, X still running; the same for the two position ranges' "
                                    f"streams): {self.tried}; nothing here can be shown")
        assert self.ctx.stream == self.S and int(self.ctx.lib.ampli_stream(self.ctx.h) or 0) == self.S.cuda_stream

    def _calibrate(self):
        """cycles of torch.cuda._sleep per millisecond, with two events; no step spins longer than twice the one before"""
        torch = self.torch
        cycles = 100_000
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0:
                return cycles / ms
            cycles *= 2

    def cycles(self, ms):
        assert ms <= MAX_DELAY_MS
        return int(ms * self.cycles_per_ms)

    def overlap(self, x, y):
        """does a tiny copy on y finish while a delay runs on x?"""
        torch = self.torch
        torch.cuda.synchronize()
        with torch.cuda.stream(x):
            torch.cuda._sleep(self.cycles(PROBE_MS))
            ev = torch.cuda.Event()
            ev.record(x)
        with torch.cuda.stream(y):
            self.tiny_d.copy_(self.tiny_h, non_blocking=True)
        y.synchronize()
        running = not ev.query()
        torch.cuda.synchronize()
        return running

    def current(self):
        """torch's current stream is the other stream: where a caller stands who calls a method outside the block the context was made in"""
        return self.torch.cuda.stream(self.other)

    def close(self):
        for c in [self.ctx, self.ctx_other] + self.rejected:
            if c is not None:
                c.close()


# ---------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------
def _np_dtype_to_torch(dt):
    import torch

    return torch.from_numpy(np.empty(0, dt)).dtype


def _alloc_out(spec):
    """an output of the caller's: whole 16-byte words (the call mask's rounding), typed view over the front"""
    import torch

    shape, dt, _ = spec
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
    raw = torch.empty(((n + 15) // 16 * 16,), dtype=torch.uint8, device="cuda")
    return raw, raw[:n].view(_np_dtype_to_torch(dt)).view(*shape)


def _fill_outs(raws, specs):
    for k, raw in raws.items():
        raw.fill_(0 if specs[k][2] == "add" else SENTINEL)


def _results_to_host(res, pinned=None):
    """device results into pinned host memory on torch's current stream (no synchronisation); host values as they are"""
    import torch

    out = {}
    for k, v in res.items():
        if isinstance(v, torch.Tensor) and v.is_cuda:
            b = _bytes(v)
            dst = pinned[k] if pinned is not None else torch.empty(b.numel(), dtype=torch.uint8).pin_memory()
            assert dst.numel() == b.numel(), (k, dst.numel(), b.numel())
            dst.copy_(b, non_blocking=True)
            out[k] = dst
        else:
            out[k] = v
    return out


def _as_numpy(host, post=None):
    import torch

    out = {}
    for k, v in host.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.numpy().copy()
        elif isinstance(v, np.ndarray):
            out[k] = np.frombuffer(v.tobytes(), np.uint8)
        else:
            out[k] = np.frombuffer(np.asarray(v).tobytes(), np.uint8)
    return post(out) if post else out


def differences(got, want):
    bad = []
    for k in want:
        if k not in got:
            bad.append(f"{k}: missing")
        elif got[k].shape != want[k].shape:
            bad.append(f"{k}: {got[k].shape} bytes, expected {want[k].shape}")
        elif not np.array_equal(got[k], want[k]):
            at = np.flatnonzero(got[k] != want[k])
            bad.append(f"{k}: {len(at)} of {len(want[k])} bytes differ, the first at {int(at[0])}")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# expected values
# ---------------------------------------------------------------------------------------------------------------------------
def reference(ref_ctx, case, world, v):
    """the case's results for variant v from the session's default-stream context: every output the caller's, pre-filled as s_delayed()
    pre-fills it -- behind a device-wide synchronisation on either side"""
    import torch

    torch.cuda.synchronize()
    x = {k: _dev(a) for k, a in case.inputs(world, v).items()}
    specs = case.outs(world) if case.outs else {}
    raws, o = {}, {}
    for k, spec in specs.items():
        raws[k], o[k] = _alloc_out(spec)
    _fill_outs(raws, specs)
    if case.setup:
        case.setup(ref_ctx)
    try:
        res = case.call(ref_ctx, x, o)
        ref_ctx.sync()
        torch.cuda.synchronize()
        host = _results_to_host(res)
        torch.cuda.synchronize()
    finally:
        if case.teardown:
            case.teardown(ref_ctx)
    return _as_numpy(host, case.post)


_EXPECTED = {}


def expected(ref_ctx, case, world):
    """(A's results, their byte sizes): computed once per case, shared, never changed.  Asserts that B's differ from A's."""
    if case.name not in _EXPECTED:
        want = reference(ref_ctx, case, world, "A")
        if case.model:
            m = {k: np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8) for k, a in case.model(case.inputs(world, "A")).items()}
            m = case.post({**want, **m}) if case.post else {**want, **m}
            bad = differences(want, {k: m[k] for k in m})
            assert not bad, f"{case.name}: the default-stream context differs from the model: {bad}"
        if not case.same_ab:
            decoy = reference(ref_ctx, case, world, "B")
            assert differences(decoy, want), f"{case.name}: the decoy's results equal the real ones: a misplaced operation would not show"
        for a in want.values():
            a.setflags(write=False)
        _EXPECTED[case.name] = want
    return _EXPECTED[case.name]


# ---------------------------------------------------------------------------------------------------------------------------
# the two modes
# ---------------------------------------------------------------------------------------------------------------------------
def _pinned_like(want):
    import torch

    return {k: torch.empty(len(a), dtype=torch.uint8).pin_memory() for k, a in want.items()}


def s_delayed(env, case, world, want, call=None):
    """mode "S delayed"; returns the list of differences (empty: the contract held)"""
    torch = env.torch
    ctx, S = env.ctx, env.S
    call = call or case.call
    A, B = case.inputs(world, "A"), case.inputs(world, "B")
    specs = case.outs(world) if case.outs else {}
    with torch.cuda.stream(S):
        x = {k: _dev(B[k]) for k in A}
        pin_a = {k: torch.from_numpy(np.ascontiguousarray(A[k]).view(np.uint8).reshape(-1).copy()).pin_memory() for k in A}
        raws, o = {}, {}
        for k, spec in specs.items():
            raws[k], o[k] = _alloc_out(spec)
        _fill_outs(raws, specs)
    pinned = _pinned_like(want)
    torch.cuda.synchronize()
    if case.setup:
        case.setup(ctx)
    try:
        with env.current():
            res = call(ctx, x, o)  # workspaces warm, on the decoy: what a stale block holds is B's
            ctx.sync()
            del res
            with torch.cuda.stream(S):
                _fill_outs(raws, specs)
            torch.cuda.synchronize()
            # ---- the measured pass ----
            t0 = time.perf_counter()
            with torch.cuda.stream(S):
                torch.cuda._sleep(env.cycles(DELAY_MS))
                delay = torch.cuda.Event()
                delay.record(S)
                for k in x:
                    _bytes(x[k]).copy_(pin_a[k], non_blocking=True)
                _fill_outs(raws, specs)
            res = call(ctx, x, o)
            with torch.cuda.stream(S):
                host = _results_to_host(res, pinned)
                ev = torch.cuda.Event()
                ev.record(S)
            pending = not ev.query() and not delay.query()  # the delay itself still runs: nothing of this pass has started
            ENQUEUE_MS[case.name, "s_delayed"] = (time.perf_counter() - t0) * 1e3
            ctx.sync()
    finally:
        torch.cuda.synchronize()
        if case.teardown:
            case.teardown(ctx)
    bad = differences(_as_numpy(host, case.post), want)
    if not case.syncs and not pending:
        bad.append(f"the delay on the stream was over before everything was enqueued: the call waited for the stream, or the host was slow (the enqueue "
                   f"took {ENQUEUE_MS[case.name, 's_delayed']:.2f} ms, the delay is {DELAY_MS} ms)")
    return bad


def other_delayed(env, case, world, want, call=None):
    """mode "other stream delayed"; returns the list of differences"""
    torch = env.torch
    ctx, S = env.ctx, env.S
    call = call or case.call
    A = case.inputs(world, "A")
    specs = {k: s for k, s in (case.outs(world) if case.outs else {}).items() if k in case.required}
    with torch.cuda.stream(S):
        x = {k: (_dev(A[k]) if k not in case.host_ok else A[k]) for k in A}
        pin_a = {k: torch.from_numpy(np.ascontiguousarray(A[k]).view(np.uint8).reshape(-1).copy()).pin_memory() for k in A if k not in case.host_ok}
        raws, o = {}, {}
        for k, spec in specs.items():
            raws[k], o[k] = _alloc_out(spec)
        _fill_outs(raws, specs)
    pinned = _pinned_like(want)
    torch.cuda.synchronize()
    if case.setup:
        case.setup(ctx)
    try:
        with env.current():
            res = call(ctx, x, o)  # workspaces warm
            ctx.sync()
            torch.cuda.synchronize()
            del res
            sizes = sorted({512} | {len(a) for a in want.values()})
            for s in (env.other, S):  # both pools: blocks of the output sizes, filled with the sentinel and freed
                with torch.cuda.stream(s):
                    blocks = [torch.empty(max(n, 1), dtype=torch.uint8, device="cuda").fill_(SENTINEL) for n in sizes for _ in range(2)]
                    del blocks
            with torch.cuda.stream(S):
                for k in pin_a:  # (a call may work in place on an input)
                    _bytes(x[k]).copy_(pin_a[k], non_blocking=True)
                _fill_outs(raws, specs)
            torch.cuda.synchronize()
            # ---- the measured pass: torch's current stream is the other stream, and it is busy ----
            t0 = time.perf_counter()
            torch.cuda._sleep(env.cycles(DELAY_MS))
            ev = torch.cuda.Event()
            ev.record(env.other)
            res = call(ctx, x, o)
            with torch.cuda.stream(ctx.stream):
                host = _results_to_host(res, pinned)
            ctx.sync()
            still = not ev.query()
            ENQUEUE_MS[case.name, "other_delayed"] = (time.perf_counter() - t0) * 1e3
            first = _as_numpy(host, case.post)
            torch.cuda.synchronize()  # the other stream has caught up: whatever waited behind its delay has now been done
            with torch.cuda.stream(ctx.stream):
                host = _results_to_host(res, pinned)
            ctx.sync()
    finally:
        torch.cuda.synchronize()
        if case.teardown:
            case.teardown(ctx)
    bad = differences(first, want)
    bad += [f"after the other stream caught up: {b}" for b in differences(_as_numpy(host, case.post), want)]  # a fill that landed on the results
    if not still:
        bad.append("the other stream's delay was over after ctx.sync(): the call waited for the other stream (an upload or a readback on it, or a "
                   "synchronisation of more than the context's stream)")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# the worlds the cases draw their inputs from (host arrays; derived inputs from the session's default-stream context)
# ---------------------------------------------------------------------------------------------------------------------------
CORE_P, CORE_S, CORE_T = 257, 5, 3
RANGE_P = 260  # two position ranges need 2 x 2 tiles of 64 positions and P a multiple of 4
SLICES = 2
SCORES_N = 1000
FLAG_DEPTH = 1 << 23  # a depth at which error_reduce raises AMPLI_FLAG_RERUN_GENERAL


class World:
    """host inputs of both variants, computed once on first use; .ctx is the session's default-stream context"""

    def __init__(self, ctx):
        self.ctx = ctx
        self._cache = {}

    def get(self, family, v):
        if (family, v) not in self._cache:
            import torch

            torch.cuda.synchronize()
            self._cache[family, v] = getattr(self, "_" + family)(v)
            self.ctx.sync()
            torch.cuda.synchronize()
        return self._cache[family, v]

    # ---- the core pass: synthetic records at P = 257, 5 normals, 3 tumours ----
    def _core(self, v):
        import torch

        from amplisolve_amd.dist import slice_geometry, slice_planes
        from tests.helpers import SEED, synth_recs, synth_ref

        ctx, P, S, T = self.ctx, CORE_P, CORE_S, CORE_T
        seed = SEED + (0 if v == "A" else 77)
        d = dict(normals=synth_recs(P, S, seed=seed), tumours=synth_recs(P, T, seed=seed, tumour=True), ref=synth_ref(P, seed=seed))
        over = d["normals"].copy()  # pack16 / pack24: a count beyond the layout in A only; flags: a depth beyond 2^22 in A only
        deep = d["normals"].copy()
        if v == "A":
            cell = np.argwhere(over[:, :, 0] > 0)[3]
            over[cell[0], cell[1], 0] = (1 << 24) + 5
            deep[cell[0], cell[1], 0] = FLAG_DEPTH
        over_b = d["normals"].copy()  # the wrong wrappers' input: a count beyond the layout in B only
        if v == "B":
            cell = np.argwhere(over_b[:, :, 0] > 0)[3]
            over_b[cell[0], cell[1], 0] = (1 << 24) + 5
        d.update(over=over, deep=deep, over_b=over_b)
        dn = _dev(d["normals"])
        acc = ctx.error_reduce(dn, P)
        fin = ctx.error_finalize(acc)
        d.update(acc=_host(acc.buf), thr=_host(fin.thr))
        parts = [ctx.error_reduce(_dev(d["normals"][a:b]), P, first_sample=a) for a, b in ((0, 3), (3, S))]
        d.update(part0=_host(parts[0].buf), part1=_host(parts[1].buf))
        pk = torch.empty(21 * P, dtype=torch.float64, device="cuda")
        ctx.acc_pack(acc, pk)
        _, gm_off, gm_bytes = ctx.regions(P)
        d.update(packed=_host(pk), regions=_host(acc.buf[gm_off: gm_off + gm_bytes]),
                 regions2=_host(torch.cat([p.buf[gm_off: gm_off + gm_bytes] for p in parts])))
        summed = ctx.new_acc(P)
        summed.buf.zero_()
        for name in ACC_SUMS:
            getattr(summed, name).copy_(sum(getattr(p, name) for p in parts))
        d.update(summed=_host(summed.buf))
        n = SLICES
        L, _, _, block_bytes = slice_geometry(P, n, False)
        pl = slice_planes(False)
        sums, gms = [], []
        for (a, b) in ((0, 3), (3, S)):
            s = torch.zeros(n * pl * L, dtype=torch.float64, device="cuda")
            g = torch.zeros(n * 8 * L, dtype=torch.float32, device="cuda")
            ctx.error_reduce_sliced(_dev(d["normals"][a:b]), P, n, s, g, first_sample=a)
            sums.append(s)
            gms.append(g)
        total = torch.stack(sums).sum(0).view(n, pl * L)
        blocks = torch.zeros(n * block_bytes, dtype=torch.uint8, device="cuda")
        for k in range(n):
            recv = torch.stack([g.view(n, 8 * L)[k] for g in gms]).contiguous()
            ctx.error_finalize_slice(P, n, k, total[k].contiguous(), recv, blocks[k * block_bytes:(k + 1) * block_bytes])
            if k == 0:
                d.update(slice_total=_host(total[0]), slice_recv=_host(recv))
        d.update(blocks=_host(blocks), slice_L=L, slice_pl=pl, block_bytes=block_bytes)
        return d

    # ---- two position ranges: the compact kernel's layout (uint16 records) at P = 260 ----
    def _ranges(self, v):
        from tests.helpers import SEED, synth_recs, synth_ref

        ctx, P = self.ctx, RANGE_P
        seed = SEED + (5 if v == "A" else 91)
        out = {}
        for name, n, tum in (("normals", CORE_S, False), ("tumours", CORE_T, True)):
            p16, fits = ctx.pack16(_dev(synth_recs(P, n, seed=seed, tumour=tum)))
            assert fits
            out[name] = _host(p16)
        out["ref"] = synth_ref(P, seed=seed)
        return out

    # ---- the records entry points: the world of tests/test_gpu_wide_offsets.py (3 rows of 130 positions, int32 records) ----
    def _wide(self, v):
        import torch

        from tests import test_gpu_wide_offsets as wo
        from tests.test_gpu_loo import _cohort as loo_cohort

        ctx, P, N = self.ctx, wo.P, wo.N
        c, h = wo._cohort(0), wo.wide_inputs()
        d = dict(recs=c["recs"], thr=c["thr"], ref=c["ref"], cls=c["cls"], m_thr=h["m_thr"], m_ref=h["m_ref"], f_thr=h["f_thr"], f_ref=h["f_ref"],
                 f_w=np.ascontiguousarray(h["f_w"], np.float32), planes_own=np.ascontiguousarray(h["planes_own"]).view(np.int64),
                 planes_pool=np.ascontiguousarray(h["planes_pool"]).view(np.int64), het_ref=np.ascontiguousarray(h["het_ref"], np.int64))
        if v == "B":  # other counts, bases, classes, thresholds, weights, genotypes: the same sets of values, elsewhere
            d["recs"] = loo_cohort(P, N, 977, u16=True)[0]
            for k in ("thr", "m_thr", "f_thr"):
                d[k] = np.ascontiguousarray(d[k][:, :, ::-1] * np.float32(1.5)).astype(np.float32)
            for k in ("ref", "cls", "m_ref", "f_ref"):
                d[k] = np.ascontiguousarray(d[k][::-1])
            d["f_w"] = (d["f_w"] * np.float32(0.5)).astype(np.float32)
            d["planes_own"], d["planes_pool"] = np.ascontiguousarray(d["planes_own"][::-1]), np.ascontiguousarray(d["planes_pool"][::-1])
            d["het_ref"] = d["het_ref"] * 2 + 1
        d["ref4"] = np.where(d["ref"] > 3, 0, d["ref"]).astype(np.uint8)
        # what indexes memory: the same in both variants
        amp_off, amp_pos = _csr32(c["amp_off"], c["amp_pos"])
        m_off, m_cell = _csr32(h["m_off"], h["m_cell"])
        f_off, f_cell = _csr32(h["f_off"], h["f_cell"])
        d.update(amp_off=amp_off, amp_pos=amp_pos, m_off=m_off, m_cell=m_cell, f_off=f_off, f_cell=f_cell, pairs=np.ascontiguousarray(h["pairs"], np.int32),
                 cand_off=np.ascontiguousarray(h["cand_off"], np.int32), cand_pos=np.ascontiguousarray(h["cand_pos"], np.int32),
                 row_g=np.ascontiguousarray(h["row_g"], np.int32), all_pairs=np.array([(i, j) for i in range(N) for j in range(N)], np.int32))
        d["meta"] = dict(P=P, N=N, cov=h["cov"], seed=h["seed"], f_cov=h["f_cov"], min_depth=h["min_depth"], min_normals=h["min_normals"])
        # derived inputs of the second-stage entry points
        rec = ctx.records(_dev(d["recs"]), "i32", N)
        acc002, acc0 = ctx.new_acc(P), ctx.new_acc(P)
        acc002.buf.zero_()
        acc0.buf.zero_()
        ctx.error_reduce_records(rec, P, acc002, 0.002, 100, summary=True)
        ctx.error_reduce_records(rec, P, acc0, 0.0, 100, summary=True)
        thr, ref, ref4 = _dev(d["thr"]), _dev(d["ref"]), _dev(d["ref4"])
        lim = ctx.detection_limits(rec, P, thr, ref, 100, ())
        disp = ctx.panel_dispersion([rec], P, acc0, 100, 4.0, samples=False)
        s2 = ctx.overdispersion_sums(rec, P, acc0, 100)
        planes = ctx.genotype_planes(rec, P)
        asums = ctx.amplicon_depth(rec, P, _dev(amp_off), _dev(amp_pos), 100)
        use = np.ones(len(amp_off) - 1, np.uint8)
        aref = ctx.amplicon_reference(asums, _dev(use), 2)
        msums, mlam = ctx.monitor_sums(rec, P, _dev(d["m_thr"]), _dev(d["m_ref"]), _dev(m_off), _dev(m_cell), cov=h["cov"])
        sites = ctx.allelic_sites(rec, P, _dev(d["planes_pool"]), _dev(d["row_g"]), _dev(d["het_ref"]), h["min_depth"], h["min_normals"], True)
        d.update(acc002=_host(acc002.buf), acc0=_host(acc0.buf), min_reads=_host(lim["min_reads"]), status=_host(lim["status"]), x2=_host(disp["x2"]),
                 rinv=_host(disp["rinv"]), d_status=_host(disp["status"]), s2=_host(s2), planes=_host(planes), asums=_host(asums), use=use,
                 aref=_host(aref["ref"]), astatus=_host(aref["status"]), msums=_host(msums), mlam=_host(mlam),
                 site_q=_host(sites[0]), site_km=_host(sites[1]), site_v=_host(sites[2]), site_code=_host(sites[3]))
        return d

    # ---- the read walks: one fuzz stream of the amplicon table (1777 reads), its mapping qualities zeroed in the decoy ----
    def _walk(self, v):
        from tests import amplicon_count_model as am
        from tests import walk_cross as wc

        s = [s for s in wc.streams("amplicon") if s.name.startswith("fuzz_28002")][0]
        buf, off = wc.staged_stream(s)  # ascending offsets, 16 readable bytes behind the last record: what all four walks take
        buf = np.ascontiguousarray(buf).copy()
        if v == "B":
            buf[off.astype(np.int64) + 13] = 0  # MAPQ: no read passes the filter
        a = am.make_amplicons(s.intervals)
        keys = np.ascontiguousarray(s.keys).view(np.int64)
        d = dict(bam=buf, rec_off=np.ascontiguousarray(off).view(np.int64), keys=keys, lo=np.ascontiguousarray(a.lo).view(np.int64).copy(),
                 hi=np.ascontiguousarray(a.hi).view(np.int64).copy(), reach=np.ascontiguousarray(a.reach).view(np.int64).copy(),
                 amp_off=np.ascontiguousarray(a.amp_off).astype(np.int64), meta=dict(mbq=s.mbq, mrq=s.mrq, min_overlap=s.min_overlap, W=int(a.amp_off[-1])))
        ctx = self.ctx
        counts, _, _ = ctx.amplicon_count(*(_dev(d[k]) for k in ("bam", "rec_off", "lo", "hi", "reach", "amp_off")), mbq=s.mbq, mrq=s.mrq, min_overlap=s.min_overlap)
        hist, _ = ctx.read_evidence(_dev(d["bam"]), _dev(d["rec_off"]), _dev(keys), mbq=s.mbq, mrq=s.mrq)
        rng = np.random.default_rng(31)
        d.update(walked=_host(counts), hist=_host(hist), ref_nt=rng.integers(0, 4, len(keys)).astype(np.int8), alt_nt=rng.integers(-1, 4, len(keys)).astype(np.int8))
        return d

    # ---- scorers, the text round trip, the FDR sort ----
    def _batch(self, v):
        from tests import fdr_planes as fp

        rng = np.random.default_rng(11 if v == "A" else 12)
        n = SCORES_N
        s = fp.case(fp.TILE_KEYS // 4 + 1, False)[0]
        return dict(k=rng.integers(1, 60, n).astype(np.int32), rd=rng.integers(100, 5000, n).astype(np.int32),
                    err=np.array([float(f"{x:f}") for x in np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), n))], np.float32),
                    x=np.exp(rng.uniform(np.log(1e-6), np.log(0.5), n)).astype(np.float32),
                    fdr_s=np.ascontiguousarray(s[0:5] if v == "A" else s[5:10]).copy())


def _pick(family, *names, **renamed):
    def inputs(world, v):
        d = world.get(family, v)
        out = {k: d[k] for k in names}
        out.update({new: d[old] for new, old in renamed.items()})
        return out

    return inputs


def _meta(world, family="wide"):
    return world.get(family, "A")["meta"]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _core_cases():
    from amplisolve_amd.api import CALL_COUNTER_STRIDE, CALL_COUNTER_WORDS, CALL_SHARDS, POISSON_FULL, POISSON_PREFILTER, Call
    from oracle import pyoracle as orc

    P, S, T = CORE_P, CORE_S, CORE_T
    CAP = 1 << 12
    acc_out = lambda w: dict(acc=((_acc_bytes(P),), np.uint8, "over"))  # noqa: E731
    list_outs = dict(call_mask=((T, P), np.uint8, "over"), calls_buf=((CAP * C.sizeof(Call),), np.uint8, "over"), n_calls=((CALL_COUNTER_WORDS,), np.int64, "over"))

    def given_acc(ctx, o):
        return _acc(ctx, P, o["acc"]) if "acc" in o else None

    def reduce_(ctx, x, o):
        return _planes(ctx.error_reduce(x["normals"], P, acc=given_acc(ctx, o)))

    def o_reduce(a):
        r = orc.error_reduce(a["normals"], P, 0.002, 100)
        return {k: r[k].astype(t) for k, t in (("snt", np.float64), ("srd", np.int64), ("cnt", np.int32), ("nrec", np.int32), ("gm_n", np.int32))}

    def estimate(ctx, x, o):
        return _table(ctx.error_estimate(x["normals"], P, out=_given_table(o)))

    def o_table(a):
        f = orc.error_finalize(orc.error_reduce(a["normals"], P, 0.002, 100))
        return dict(thr=f["thr"].astype(np.float32), code=f["code"].astype(np.uint8))

    def finalize(ctx, x, o):
        return _table(ctx.error_finalize(_acc(ctx, P, x["acc"]), out=_given_table(o)))

    def inorder(ctx, x, o):
        acc = given_acc(ctx, o) or ctx.new_acc(P)
        ctx.error_sums_inorder(ctx.records(x["normals"], "i32", S), P, acc)
        return dict(snt=acc.snt)

    def reduce_records(ctx, x, o):
        acc = given_acc(ctx, o) or ctx.new_acc(P)
        fin = ctx.error_reduce_records(ctx.records(x["normals"], "i32", S), P, acc, finalize=True, out=_given_table(o))
        return {**_planes(acc), **_table(fin)}

    def counters(res):
        return res["n_calls"][::CALL_COUNTER_STRIDE]

    def given_list(o):
        return {k: o[k] for k in ("call_mask", "calls_buf", "n_calls") if k in o}

    def call_prefilter(ctx, x, o):
        res = ctx.poisson_call(x["tumours"], P, x["thr"], x["ref"], 100, mode=POISSON_PREFILTER, capacity=CAP, **given_list(o))
        return dict(call_mask=res["call_mask"], counters=counters(res))

    def o_call(a):
        return dict(call_mask=orc.poisson_call(a["tumours"], P, a["thr"], a["ref"], 100, dense=False)["call_mask"].astype(np.uint8))

    def call_drained_aside(ctx, x, o):
        res = ctx.poisson_call(x["tumours"], P, x["thr"], x["ref"], 100, mode=POISSON_PREFILTER, capacity=CAP, **given_list(o))
        ctx.wait_calls()  # "the context's stream waits, the host does not block"
        return dict(call_mask=res["call_mask"], counters=counters(res))

    def call_all_scores(ctx, x, o):
        kw = {k: o[k] for k in ("call_mask", "q", "af") if k in o}
        res = ctx.poisson_call(x["tumours"], P, x["thr"], x["ref"], 100, mode=POISSON_FULL, dense_q="q" not in o, dense_af="af" not in o, **kw)
        return dict(call_mask=res["call_mask"], q=res["q"], af=res["af"])

    def call_blocks(ctx, x, o):
        res = ctx.poisson_call(x["tumours"], P, x["blocks"], x["ref"], 100, mode=POISSON_PREFILTER, capacity=CAP, blocks_of=SLICES, **given_list(o))
        return dict(call_mask=res["call_mask"], counters=counters(res))

    def call_records(ctx, x, o):
        res = ctx.poisson_call_records(ctx.records(x["tumours"], "i32", T), P, x["thr"], x["ref"], 100, mode=POISSON_PREFILTER, capacity=CAP, **given_list(o))
        return dict(call_mask=res["call_mask"], counters=counters(res))

    def read_calls(ctx, x, o):
        res = ctx.poisson_call(x["tumours"], P, x["thr"], x["ref"], 100, mode=POISSON_PREFILTER, capacity=CAP, **given_list(o))
        calls = ctx.read_calls(res)
        return dict(calls=calls, total=ctx.n_calls_total(res))

    def flags(ctx, x, o):
        ctx.error_reduce(x["deep"], P)
        return dict(flags=ctx.flags())

    def pack(layout):
        def call(ctx, x, o):
            out, fits = (ctx.pack16 if layout == "u16" else ctx.pack24)(x["over"])
            return dict(fits=bool(fits))

        return call

    def packed_(ctx, x, o):
        acc = given_acc(ctx, o) or ctx.new_acc(P)
        ctx.error_reduce_packed(x["normals"], P, acc, o["packed"])
        return dict(packed=o["packed"], gm_n=acc.gm_n)

    def finalize_merged(ctx, x, o):
        return _table(ctx.error_finalize_merged(P, x["packed"], x["regions"], 1, out=_given_table(o)))

    def merge(ctx, x, o):
        return _planes(ctx.acc_merge([_acc(ctx, P, x["part0"]), _acc(ctx, P, x["part1"])], dst=given_acc(ctx, o)))

    def acc_pack(ctx, x, o):
        ctx.acc_pack(_acc(ctx, P, x["acc"]), o["packed"])
        return dict(packed=o["packed"])

    def acc_unpack(ctx, x, o):
        acc = _acc(ctx, P, o["acc"])
        ctx.acc_unpack(x["packed"], acc)
        return _planes(acc, ACC_SUMS)

    def gm_merge(ctx, x, o):
        acc = _acc(ctx, P, x["summed"])
        ctx.gm_merge(acc, x["regions2"], 2)
        return _planes(acc)

    def sliced_outs(w):
        d = w.get("core", "A")
        return dict(sums=((SLICES * d["slice_pl"] * d["slice_L"],), np.float64, "over"), gm=((SLICES * 8 * d["slice_L"],), np.float32, "over"))

    def reduce_sliced(ctx, x, o):
        ctx.error_reduce_sliced(x["normals"], P, SLICES, o["sums"], o["gm"])
        return dict(sums=o["sums"], gm=o["gm"])

    def reduce_records_sliced(ctx, x, o):
        ctx.error_reduce_records_sliced(ctx.records(x["normals"], "i32", S), P, None, SLICES, o["sums"], o["gm"])
        return dict(sums=o["sums"], gm=o["gm"])

    def finalize_slice(ctx, x, o):
        ctx.error_finalize_slice(P, SLICES, 0, x["slice_total"], x["slice_recv"], o["block"])
        return dict(block=o["block"])

    def unslice(ctx, x, o):
        return _table(ctx.error_table_unslice(P, SLICES, x["blocks"], out=_given_table(o)))

    def synth(ctx, x, o):
        return dict(recs=ctx.synth_fill(P, S, out=o.get("recs")), tumours=ctx.synth_fill(P, T, tumour=True), ref=ctx.synth_ref(P))

    def o_synth(a):
        from tests.helpers import synth_recs, synth_ref

        return dict(recs=synth_recs(P, S), tumours=synth_recs(P, T, tumour=True), ref=synth_ref(P))

    def ranges_setup(ctx):
        ctx.set_record_layout("u16")
        ctx.set_ranges(2)

    def ranges_teardown(ctx):
        ctx.set_ranges(1)
        ctx.set_record_layout("i32")

    RP = RANGE_P

    def ranged(ctx, x, o):
        fin = ctx.error_estimate(x["normals"], RP, out=_given_table(o))
        kw = {k[2:]: o[k] for k in ("r_call_mask", "r_calls_buf", "r_n_calls") if k in o}
        res = ctx.poisson_call(x["tumours"], RP, fin.thr, x["ref"], 100, mode=POISSON_PREFILTER, capacity=CAP, **kw)
        ctx.ranges_join()  # the context's stream waits for every range
        return {**_table(fin), "call_mask": res["call_mask"], "counters": counters(res)}

    def ranged_outs(w):
        return {**_table_outs(RP), "r_call_mask": ((T, RP), np.uint8, "over"), "r_calls_buf": ((CAP * C.sizeof(Call),), np.uint8, "over"),
                "r_n_calls": ((CALL_COUNTER_WORDS,), np.int64, "over")}

    assert CAP % CALL_SHARDS == 0
    core = functools.partial(_pick, "core")
    drain_on, drain_off = (lambda ctx: ctx.set_async_drain(True)), (lambda ctx: ctx.set_async_drain(False))
    return [
        Case("error_reduce", ("error_reduce", "new_acc"), core("normals"), reduce_, acc_out, model=o_reduce),
        Case("error_estimate", ("error_estimate",), core("normals"), estimate, lambda w: _table_outs(P), post=post_table, model=o_table),
        Case("error_finalize", ("error_finalize",), core("acc"), finalize, lambda w: _table_outs(P), post=post_table),
        Case("error_sums_inorder", ("error_sums_inorder",), core("normals"), inorder, acc_out),
        Case("error_reduce_records", ("error_reduce_records",), core("normals"), reduce_records, lambda w: {**acc_out(w), **_table_outs(P)}, post=post_table),
        Case("poisson_call/prefilter", ("poisson_call",), core("tumours", "thr", "ref"), call_prefilter, lambda w: list_outs, model=o_call),
        Case("poisson_call/all_scores", ("poisson_call",), core("tumours", "thr", "ref"), call_all_scores,
             lambda w: dict(call_mask=((T, P), np.uint8, "over"), q=((T, P, 4, 2), np.float64, "over"), af=((T, P, 4, 3), np.float32, "over"))),
        Case("poisson_call/async_drain", ("poisson_call", "wait_calls", "set_async_drain"), core("tumours", "thr", "ref"), call_drained_aside, lambda w: list_outs,
             setup=drain_on, teardown=drain_off, model=o_call),
        Case("poisson_call/two_ranges", ("poisson_call", "error_estimate", "set_ranges", "ranges_join"), _pick("ranges", "normals", "tumours", "ref"), ranged,
             ranged_outs, setup=ranges_setup, teardown=ranges_teardown, post=post_table),
        Case("poisson_call/blocks", ("poisson_call",), core("tumours", "blocks", "ref"), call_blocks, lambda w: list_outs),
        Case("poisson_call_records", ("poisson_call_records",), core("tumours", "thr", "ref"), call_records, lambda w: list_outs, model=o_call),
        Case("read_calls", ("read_calls", "n_calls_total"), core("tumours", "thr", "ref"), read_calls, lambda w: list_outs, syncs=SYNC_HOST),
        Case("flags", ("flags",), core("deep"), flags, syncs=SYNC_FLAGS),
        Case("pack16", ("pack16",), core("over"), pack("u16"), syncs=SYNC_HOST),
        Case("pack24", ("pack24",), core("over"), pack("u24"), syncs=SYNC_HOST),
        Case("error_reduce_packed", ("error_reduce_packed",), core("normals"), packed_, lambda w: {**acc_out(w), "packed": ((21 * P,), np.float64, "over")},
             required=("packed",)),
        Case("error_finalize_merged", ("error_finalize_merged",), core("packed", "regions"), finalize_merged, lambda w: _table_outs(P), post=post_table),
        Case("acc_merge", ("acc_merge",), core("part0", "part1"), merge, acc_out, syncs=SYNC_MERGE),
        Case("acc_pack", ("acc_pack",), core("acc"), acc_pack, lambda w: dict(packed=((21 * P,), np.float64, "over")), required=("packed",)),
        Case("acc_unpack", ("acc_unpack",), core("packed"), acc_unpack, acc_out, required=("acc",)),
        Case("gm_merge", ("gm_merge",), core("summed", "regions2"), gm_merge),
        Case("error_reduce_sliced", ("error_reduce_sliced",), core("normals"), reduce_sliced, sliced_outs, required=("sums", "gm")),
        Case("error_reduce_records_sliced", ("error_reduce_records_sliced",), core("normals"), reduce_records_sliced, sliced_outs, required=("sums", "gm")),
        Case("error_finalize_slice", ("error_finalize_slice",), core("slice_total", "slice_recv"), finalize_slice,
             lambda w: dict(block=((w.get("core", "A")["block_bytes"],), np.uint8, "over")), required=("block",)),
        Case("error_table_unslice", ("error_table_unslice",), core("blocks"), unslice, lambda w: _table_outs(P), post=post_table),
        Case("synth", ("synth_fill", "synth_ref"), lambda w, v: {}, synth, lambda w: dict(recs=((S, P, 8), np.int32, "over")), model=o_synth, same_ab=True),
    ]


def _records_cases():
    from amplisolve_amd.api import (AI_SUMS, AMP_SUMS, CALL_COUNTER_STRIDE, CALL_SHARDS, CALL_COUNTER_WORDS, CONTAM_SUMS, GENO_PLANES, LIMIT_COUNTERS, MON_SUMS,
                                    POISSON_PREFILTER, SPEC_SUMS, TF_COUNTS, TF_VALS, DiluteMix, LooCall)
    from tests.test_gpu_wide_offsets import LEVELS
    from tests.test_gpu_wide_offsets import N as N_
    from tests.test_gpu_wide_offsets import P as P_

    P, N = P_, N_
    W64 = (P + 63) // 64
    wide = functools.partial(_pick, "wide")
    CAP = CALL_SHARDS * 4 * N * P  # every shard holds every cell: no segment can overflow, whichever variant the kernel reads

    def rec(ctx, x, name="recs"):
        return ctx.records(x[name], "i32", N)

    def given(o, *names):
        return {k: o[k] for k in names if k in o}

    def loo(ctx, x, o):
        res = ctx.loo_call(rec(ctx, x), P, _acc(ctx, P, x["acc002"]), x["ref"], 0.002, 100, 100, mode=POISSON_PREFILTER, capacity=CAP, dense_thr=True,
                           **given(o, "call_mask", "calls_buf", "n_calls", "callable_pos", "callable_sample", "flags", "thr_loo"))
        return dict(call_mask=res["call_mask"], callable_pos=res["callable_pos"], callable_sample=res["callable_sample"], thr_loo=res["thr_loo"], flags=res["flags"],
                    counters=res["n_calls"][::CALL_COUNTER_STRIDE])

    loo_outs = dict(call_mask=((N, P), np.uint8, "over"), calls_buf=((CAP * C.sizeof(LooCall),), np.uint8, "over"), n_calls=((CALL_COUNTER_WORDS,), np.int64, "over"),
                    callable_pos=((P,), np.int32, "add"), callable_sample=((N,), np.int32, "add"), flags=((1,), np.int32, "add"), thr_loo=((N, 2, 4, P), np.float32, "over"))

    def read_loo(ctx, x, o):
        res = ctx.loo_call(rec(ctx, x), P, _acc(ctx, P, x["acc002"]), x["ref"], 0.002, 100, 100, mode=POISSON_PREFILTER, capacity=CAP,
                           **given(o, "call_mask", "calls_buf", "n_calls", "callable_pos", "callable_sample", "flags"))
        return dict(calls=ctx.read_loo_calls(res))

    def limits(ctx, x, o):
        res = ctx.detection_limits(rec(ctx, x), P, x["thr"], x["ref"], 100, LEVELS, **given(o, "counts"))
        return dict(min_reads=res["min_reads"], status=res["status"], counts=res["counts"])

    def limit_stats(ctx, x, o):
        ctx.limit_stats(reset=True)
        ctx.detection_limits(rec(ctx, x), P, x["thr"], x["ref"], 100, LEVELS)
        return dict(stats=np.array(ctx.limit_stats(), np.int64))

    def power(ctx, x, o):
        res = ctx.detection_power(rec(ctx, x), P, x["min_reads"], x["status"], LEVELS, 0.95, **given(o, "counts"))
        return dict(power=res["power"], lod=res["lod"], counts=res["counts"])

    def power_stats(ctx, x, o):
        ctx.power_stats(reset=True)
        ctx.detection_power(rec(ctx, x), P, x["min_reads"], x["status"], LEVELS, 0.95)
        return dict(stats=np.array(ctx.power_stats(), np.int64))

    def dispersion(ctx, x, o):
        ctx.dispersion_records(rec(ctx, x), P, _acc(ctx, P, x["acc0"]), 100, o["x2"], o["rinv"], False, o["sx"], o["se"], o["st"])
        return dict(o)

    disp_outs = dict(x2=((2, 4, P), np.float64, "over"), rinv=((2, 4, P), np.float64, "over"), sx=((N,), np.float64, "over"), se=((N,), np.float64, "over"),
                     st=((N,), np.int64, "over"))

    def dispersion_finalize(ctx, x, o):
        ctx.dispersion_finalize(P, _acc(ctx, P, x["acc0"]), x["x2"], x["rinv"], 4.0, o["z"], o["phi"], o["status"], o["counts"])
        return dict(o)

    dfin_outs = dict(z=((2, 4, P), np.float64, "over"), phi=((2, 4, P), np.float32, "over"), status=((2, 4, P), np.uint8, "over"), counts=((4,), np.int64, "add"))

    def panel_dispersion(ctx, x, o):
        res = ctx.panel_dispersion([rec(ctx, x)], P, _acc(ctx, P, x["acc0"]), 100, 4.0, samples=True)
        return {k: res[k] for k in ("x2", "rinv", "z", "phi", "status", "counts", "sample_x2", "sample_expect", "sample_terms")}

    def genotype(ctx, x, o):
        return dict(planes=ctx.genotype_planes(rec(ctx, x), P, **given(o, "out")))

    def concordance(ctx, x, o):
        return dict(counts=ctx.concordance(x["planes"], x["planes_pool"], P))

    def contamination(ctx, x, o):
        return dict(sums=ctx.contamination(rec(ctx, x), P, x["planes"], x["planes_pool"], **given(o, "out")))

    def amplicon_depth(ctx, x, o):
        return dict(sums=ctx.amplicon_depth(rec(ctx, x), P, x["amp_off"], x["amp_pos"], 100, **given(o, "out")))

    def amplicon_reference(ctx, x, o):
        r = ctx.amplicon_reference(x["asums"], x["use"], 2)
        return dict(total=r["total"], ref=r["ref"], status=r["status"])

    def amplicon_ratio(ctx, x, o):
        r = ctx.amplicon_ratio(x["asums"], x["use"], dict(ref=x["aref"], status=x["astatus"]))
        return dict(r)

    def spectrum(ctx, x, o):
        return dict(sums=ctx.spectrum(rec(ctx, x), P, x["ref"], x["cls"], 5, 100, 1000, **given(o, "out")))

    def exceedance(ctx, x, o):
        e, g = ctx.exceedance(rec(ctx, x), rec(ctx, x), P, x["ref4"], 100, 100, **given(o, "elig", "ge"))
        return dict(elig=e, ge=g)

    def od_sums(ctx, x, o):
        return dict(s2=ctx.overdispersion_sums(rec(ctx, x), P, _acc(ctx, P, x["acc0"]), 100, **given(o, "s2")))

    def od_fit(ctx, x, o):
        return dict(omega=ctx.overdispersion_fit(P, _acc(ctx, P, x["acc0"]), x["x2"], x["s2"], x["d_status"], **given(o, "omega")))

    def nb_score(ctx, x, o):
        return dict(q=ctx.nb_score(rec(ctx, x), P, x["thr"], x["ref4"], None, 100, **given(o, "q")))

    def pair_score(ctx, x, o):
        return dict(s=ctx.pair_score(rec(ctx, x), rec(ctx, x), P, x["all_pairs"], x["ref4"], 30, **given(o, "s")))

    def mixtures(v):
        from tests.dilution_model import KEEP_ALL, keep_of

        f = (lambda a: a) if v == "A" else (lambda a: min(1.0, a * 0.5 + 0.05))
        mix = [(0, 1, keep_of(f(0.3)), keep_of(f(0.7)), 11), (1, 2, keep_of(f(0.5)), KEEP_ALL, 12), (2, 0, KEEP_ALL, keep_of(f(0.1)), 13),
               (2, 2, keep_of(f(0.9)), keep_of(f(0.9)), 14), (1, -1, keep_of(f(0.25)), 0, 15)]
        rows = [DiluteMix(int(ra), int(rb), int(ka), int(kb), int(key) + (0 if v == "A" else 100)) for ra, rb, ka, kb, key in mix]
        return np.frombuffer(bytes((DiluteMix * len(rows))(*rows)), np.uint8).reshape(len(rows), C.sizeof(DiluteMix)).copy()

    def dilute_inputs(world, v):
        return dict(recs=world.get("wide", v)["recs"], mix=mixtures(v))

    def dilute(ctx, x, o):
        mix = x["mix"]
        if isinstance(mix, np.ndarray):  # the host form: a sequence of (row_a, row_b, keep_a, keep_b, key)
            m = (DiluteMix * len(mix)).from_buffer_copy(mix.tobytes())
            mix = [(r.row_a, r.row_b, r.keep_a, r.keep_b, r.key) for r in m]
        out, fl = ctx.dilute(rec(ctx, x), rec(ctx, x), P, mix, **given(o, "out", "flags"))
        return dict(out=out, flags=fl)

    def monitor_sums(ctx, x, o):
        m = _meta_of(x)
        s, l = ctx.monitor_sums(rec(ctx, x), P, x["m_thr"], x["m_ref"], x["m_off"], x["m_cell"], cov=m["cov"], **given(o, "sums", "lam"))
        return dict(sums=s, lam=l)

    def monitor_controls(ctx, x, o):
        m = _meta_of(x)
        s, l = ctx.monitor_controls(rec(ctx, x), P, x["m_thr"], x["m_ref"], x["m_off"], x["m_cell"], x["pairs"], x["cand_off"], x["cand_pos"], 3, first_rep=2,
                                    seed=m["seed"], cov=m["cov"], **given(o, "sums", "lam"))
        return dict(sums=s, lam=l)

    def monitor_score(ctx, x, o):
        return dict(q=ctx.monitor_score(x["msums"], x["mlam"], **given(o, "q")))

    def fraction(ctx, x, o):
        m = _meta_of(x)
        est, count = ctx.tumour_fraction(rec(ctx, x), P, x["f_thr"], x["f_ref"], x["f_off"], x["f_cell"], x["f_w"], cov=m["f_cov"], **given(o, "est", "count"))
        return dict(est=est, count=count)

    def hetsite(ctx, x, o):
        return dict(ref=ctx.hetsite_reference(rec(ctx, x), P, x["planes_own"], _meta_of(x)["min_depth"], **given(o, "ref")))

    def sites(ctx, x, o):
        m = _meta_of(x)
        q, km, v, code = ctx.allelic_sites(rec(ctx, x), P, x["planes_pool"], x["row_g"], x["het_ref"], m["min_depth"], m["min_normals"], True,
                                           **given(o, "q", "km", "v", "code"))
        return dict(q=q, km=km, v=v, code=code)

    def regions(ctx, x, o):
        return dict(sums=ctx.allelic_regions(x["site_q"], x["site_km"], x["site_v"], x["site_code"], x["amp_off"], x["amp_pos"], 20.0, **given(o, "out")))

    meta = {}

    def _meta_of(x):
        return meta["m"]

    def with_meta(inputs):
        def f(world, v):
            meta["m"] = _meta(world)
            return inputs(world, v)

        return f

    def n_lists(w, off):
        return len(w.get("wide", "A")[off]) - 1

    def n_of(w, key):
        return len(w.get("wide", "A")[key])

    return [
        Case("loo_call", ("loo_call",), wide("recs", "acc002", "ref"), loo, lambda w: loo_outs),
        Case("read_loo_calls", ("read_loo_calls",), wide("recs", "acc002", "ref"), read_loo, lambda w: {k: v for k, v in loo_outs.items() if k != "thr_loo"}, syncs=SYNC_HOST),
        Case("detection_limits", ("detection_limits",), wide("recs", "thr", "ref"), limits, lambda w: dict(counts=((N, LIMIT_COUNTERS + len(LEVELS)), np.int64, "add"))),
        Case("limit_stats", ("limit_stats",), wide("recs", "thr", "ref"), limit_stats, syncs=SYNC_LIMIT),
        Case("detection_power", ("detection_power",), wide("recs", "min_reads", "status"), power, lambda w: dict(counts=((N, 1 + len(LEVELS)), np.int64, "add"))),
        Case("power_stats", ("power_stats",), wide("recs", "min_reads", "status"), power_stats, syncs=SYNC_POWER),
        Case("dispersion_records", ("dispersion_records",), wide("recs", "acc0"), dispersion, lambda w: disp_outs, required=tuple(disp_outs)),
        Case("dispersion_finalize", ("dispersion_finalize",), wide("acc0", "x2", "rinv"), dispersion_finalize, lambda w: dfin_outs, required=tuple(dfin_outs)),
        Case("panel_dispersion", ("panel_dispersion",), wide("recs", "acc0"), panel_dispersion),
        Case("genotype_planes", ("genotype_planes",), wide("recs"), genotype, lambda w: dict(out=((N, GENO_PLANES, W64), np.int64, "over"))),
        Case("concordance", ("concordance",), wide("planes", "planes_pool"), concordance),
        Case("contamination", ("contamination",), wide("recs", "planes", "planes_pool"), contamination, lambda w: dict(out=((N, 12, CONTAM_SUMS), np.int64, "over"))),
        Case("amplicon_depth", ("amplicon_depth",), wide("recs", "amp_off", "amp_pos"), amplicon_depth,
             lambda w: dict(out=((N, n_lists(w, "amp_off"), AMP_SUMS), np.int64, "over")), host_ok=("amp_off", "amp_pos")),
        Case("amplicon_reference", ("amplicon_reference",), wide("asums", "use"), amplicon_reference),
        Case("amplicon_ratio", ("amplicon_ratio",), wide("asums", "use", "aref", "astatus"), amplicon_ratio),
        Case("spectrum", ("spectrum",), wide("recs", "ref", "cls"), spectrum, lambda w: dict(out=((N, 5, SPEC_SUMS), np.int64, "over")), host_ok=("ref", "cls")),
        Case("exceedance", ("exceedance",), wide("recs", "ref4"), exceedance, lambda w: dict(elig=((N, P), np.int16, "over"), ge=((N, P, 4, 2), np.int16, "over")),
             host_ok=("ref4",)),
        Case("overdispersion_sums", ("overdispersion_sums",), wide("recs", "acc0"), od_sums, lambda w: dict(s2=((2, 4, P), np.float64, "over"))),
        Case("overdispersion_fit", ("overdispersion_fit",), wide("acc0", "x2", "s2", "d_status"), od_fit, lambda w: dict(omega=((2, 4, P), np.float64, "over"))),
        Case("nb_score", ("nb_score",), wide("recs", "thr", "ref4"), nb_score, lambda w: dict(q=((N, P, 4, 2), np.float32, "over"))),
        Case("pair_score", ("pair_score",), wide("recs", "all_pairs", "ref4"), pair_score, lambda w: dict(s=((N * N, P, 4, 2), np.float32, "over"))),
        Case("dilute", ("dilute",), dilute_inputs, dilute, lambda w: dict(out=((5, P, 8), np.int32, "over"), flags=((5,), np.int32, "over")), host_ok=("mix",)),
        Case("monitor_sums", ("monitor_sums",), with_meta(wide("recs", "m_thr", "m_ref", "m_off", "m_cell")), monitor_sums,
             lambda w: dict(sums=((N, n_lists(w, "m_off"), MON_SUMS), np.int64, "over"), lam=((N, n_lists(w, "m_off"), 2), np.float64, "over")), host_ok=("m_off", "m_cell")),
        Case("monitor_controls", ("monitor_controls",), with_meta(wide("recs", "m_thr", "m_ref", "m_off", "m_cell", "pairs", "cand_off", "cand_pos")), monitor_controls,
             lambda w: dict(sums=((n_of(w, "pairs"), 3, MON_SUMS), np.int64, "over"), lam=((n_of(w, "pairs"), 3, 2), np.float64, "over")), host_ok=("m_off", "m_cell")),
        Case("monitor_score", ("monitor_score",), wide("msums", "mlam"), monitor_score, lambda w: dict(q=((N, n_lists(w, "m_off"), 2), np.float32, "over"))),
        Case("tumour_fraction", ("tumour_fraction",), with_meta(wide("recs", "f_thr", "f_ref", "f_off", "f_cell", "f_w")), fraction,
             lambda w: dict(est=((N, n_lists(w, "f_off"), TF_VALS), np.float64, "over"), count=((N, n_lists(w, "f_off"), TF_COUNTS), np.int64, "over")),
             host_ok=("f_off", "f_cell", "f_w")),
        Case("hetsite_reference", ("hetsite_reference",), with_meta(wide("recs", "planes_own")), hetsite, lambda w: dict(ref=((3, 6, P), np.int64, "add"))),
        Case("allelic_sites", ("allelic_sites",), with_meta(wide("recs", "planes_pool", "row_g", "het_ref")), sites,
             lambda w: dict(q=((N, P), np.float32, "over"), km=((N, P, 2), np.int32, "over"), v=((N, P), np.float64, "over"), code=((N, P), np.uint8, "over"))),
        Case("allelic_regions", ("allelic_regions",), wide("site_q", "site_km", "site_v", "site_code", "amp_off", "amp_pos"), regions,
             lambda w: dict(out=((N, n_lists(w, "amp_off"), AI_SUMS), np.int64, "over")), host_ok=("amp_off", "amp_pos")),
    ]


def _walk_cases():
    from amplisolve_amd.api import EVIDENCE_BINS, EVIDENCE_METRICS, INDEL_LEN_BINS

    walk = functools.partial(_pick, "walk")
    m = {}

    def with_meta(inputs):
        def f(world, v):
            m.update(_meta(world, "walk"))
            return inputs(world, v)

        return f

    def given(o, *names):
        return {k: o[k] for k in names if k in o}

    def n_keys(w):
        return len(w.get("walk", "A")["keys"])

    def n_amp(w):
        return len(w.get("walk", "A")["lo"])

    def pileup(ctx, x, o):
        ctx._check(ctx.lib.ampli_pileup_count(ctx.h, x["bam"].data_ptr(), x["rec_off"].data_ptr(), x["rec_off"].numel(), x["keys"].data_ptr(), x["keys"].numel(),
                                              m["mbq"], m["mrq"], o["counts"].data_ptr(), o["stats"].data_ptr()))
        return dict(o)

    def indel(ctx, x, o):
        c, l, s = ctx.indel_count(x["bam"], x["rec_off"], x["keys"], mbq=m["mbq"], mrq=m["mrq"], **given(o, "counts", "lengths", "stats"))
        return dict(counts=c, lengths=l, stats=s)

    def evidence(ctx, x, o):
        h, s = ctx.read_evidence(x["bam"], x["rec_off"], x["keys"], mbq=m["mbq"], mrq=m["mrq"], **given(o, "hist", "stats"))
        return dict(hist=h, stats=s)

    def amplicon(ctx, x, o):
        c, r, s = ctx.amplicon_count(x["bam"], x["rec_off"], x["lo"], x["hi"], x["reach"], x["amp_off"], mbq=m["mbq"], mrq=m["mrq"], min_overlap=m["min_overlap"],
                                     **given(o, "counts", "amp_reads", "stats"))
        return dict(counts=c, amp_reads=r, stats=s)

    def layers(ctx, x, o):
        l, a, t = ctx.amplicon_layers(x["walked"], x["lo"], x["hi"], x["reach"], x["amp_off"], x["keys"], L=2, **given(o, "layers", "layer_amp", "total"))
        return dict(layers=l, layer_amp=a, total=t)

    def score(ctx, x, o):
        i, md, z2, used = ctx.evidence_score(x["hist"], x["ref_nt"], x["alt_nt"], **given(o, "ints", "med", "z2", "alt_used"))
        return dict(ints=i, med=md, z2=z2, alt_used=used)

    return [
        Case("pileup_count", (), with_meta(walk("bam", "rec_off", "keys")), pileup, lambda w: dict(counts=((n_keys(w), 8), np.int32, "add"), stats=((2,), np.int64, "add")),
             required=("counts", "stats"), protos=("ampli_pileup_count",)),
        Case("indel_count", ("indel_count",), with_meta(walk("bam", "rec_off", "keys")), indel,
             lambda w: dict(counts=((n_keys(w), 8), np.int32, "add"), lengths=((n_keys(w), 2, INDEL_LEN_BINS), np.int32, "add"), stats=((2,), np.int64, "add"))),
        Case("read_evidence", ("read_evidence",), with_meta(walk("bam", "rec_off", "keys")), evidence,
             lambda w: dict(hist=((n_keys(w), 4, EVIDENCE_METRICS, EVIDENCE_BINS), np.int32, "add"), stats=((2,), np.int64, "add"))),
        Case("amplicon_count", ("amplicon_count",), with_meta(walk("bam", "rec_off", "lo", "hi", "reach", "amp_off")), amplicon,
             lambda w: dict(counts=((w.get("walk", "A")["meta"]["W"], 8), np.int32, "add"), amp_reads=((n_amp(w), 2), np.int64, "add"), stats=((4,), np.int64, "add"))),
        Case("amplicon_layers", ("amplicon_layers",), with_meta(walk("walked", "lo", "hi", "reach", "amp_off", "keys")), layers,
             lambda w: dict(layers=((2, n_keys(w), 8), np.int32, "over"), layer_amp=((2, n_keys(w)), np.int32, "over"), total=((n_keys(w), 8), np.int32, "over"))),
        Case("evidence_score", ("evidence_score",), walk("hist", "ref_nt", "alt_nt"), score,
             lambda w: dict(ints=((n_keys(w), EVIDENCE_METRICS, 3), np.int64, "over"), med=((n_keys(w), EVIDENCE_METRICS, 2), np.int32, "over"),
                            z2=((n_keys(w), EVIDENCE_METRICS), np.float64, "over"), alt_used=((n_keys(w),), np.int8, "over"))),
    ]


def _batch_cases():
    from tests import fdr_planes as fp

    batch = functools.partial(_pick, "batch")
    FP = fp.TILE_KEYS // 4 + 1

    def score(ctx, x, o):
        q, p = ctx.score_batch(x["k"], x["rd"], x["err"])
        return dict(q=q, p=p)

    def dense(ctx, x, o):
        return dict(q=ctx.score_dense_batch(x["k"], x["rd"], x["err"]))

    def drain(ctx, x, o):
        q, p = ctx.drain_score_batch(x["k"], x["rd"], x["err"])
        return dict(q=q, p=p)

    def roundtrip(ctx, x, o):
        return dict(out=ctx.roundtrip_batch(x["x"]))

    def fdr(ctx, x, o):
        kw = {k: o[k] for k in ("a", "m", "rank") if k in o}
        kw.setdefault("rank", True)
        a, mm, r = ctx.fdr_adjust(x["fdr_s"], False, **kw)
        return dict(a=a, m=mm, rank=r)

    return [
        Case("score_batch", ("score_batch",), batch("k", "rd", "err"), score),
        Case("score_dense_batch", ("score_dense_batch",), batch("k", "rd", "err"), dense),
        Case("drain_score_batch", ("drain_score_batch",), batch("k", "rd", "err"), drain),
        Case("roundtrip_batch", ("roundtrip_batch",), batch("x"), roundtrip),
        Case("fdr_adjust", ("fdr_adjust", "fdr_workspace_bytes"), batch("fdr_s"), fdr,
             lambda w: dict(a=((5, FP, 4), np.float32, "over"), m=((5,), np.int32, "over"), rank=((5, FP, 4), np.int32, "over"))),
    ]


@functools.lru_cache(None)
def cases():
    out = _core_cases() + _records_cases() + _walk_cases() + _batch_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return [c for c in cases() if c.name == name][0]


# ---------------------------------------------------------------------------------------------------------------------------
# what is no case, and why (tests/test_stream_order_complete.py: a method or entry point that is neither fails there)
# ---------------------------------------------------------------------------------------------------------------------------
SETTER = "a setting of the context: host state, no device operation of its own (a case runs under it where it changes what is launched)"
GETTER = "reads host state of the context or of the library: no device operation"
EVENT = "an event handle or a record on the context's stream by the library itself: nothing of torch's to place"
GRAPH = "a hipGraph handle: capture and replay are held to the stream, for the outputs the caller brings, by the two hipGraph tests (tests/test_gpu_parity.py, tests/test_gpu_output_contracts.py)"
ALLOC = "allocation, registration or a raw copy for callers without torch: Context has no method over it"
POINTERS = "wraps the pointers of the caller's tensors in a struct on the host: no device operation"
COMM = "needs a communicator, and no second GPU is available"
LIFE = "creates, destroys or synchronises the context"

EXEMPT_METHODS = {
    "close": LIFE, "sync": LIFE,
    "records": POINTERS, "dilution_records": POINTERS, "pack": "dispatches to pack16 / pack24, which are cases",
    "set_record_layout": SETTER, "set_tuning": SETTER, "set_reduce_compact": SETTER, "set_slice_format": SETTER, "set_poisson_tuning": SETTER,
    "set_queue_items": SETTER, "set_slice_group": SETTER,
    "last_reduce_kernel": GETTER, "ranges_concurrent": GETTER, "last_spectrum_segments": GETTER, "slice_len": GETTER, "regions": GETTER, "elapsed_ms": GETTER,
    "event": EVENT, "record": EVENT, "range_record": EVENT,
    "graph_begin": GRAPH, "graph_end": GRAPH, "graph_launch": GRAPH, "graph_destroy": GRAPH,
}

EXEMPT_PROTOS = {
    "ampli_ctx_destroy": LIFE, "ampli_sync": LIFE, "ampli_last_error": GETTER, "ampli_stream": GETTER,
    "ampli_host_register": ALLOC, "ampli_dev_alloc": ALLOC, "ampli_dev_free": ALLOC, "ampli_copy_h2d": ALLOC, "ampli_copy_d2h": ALLOC, "ampli_memset_d": ALLOC,
    "ampli_mem_info": GETTER, "ampli_acc_to_slices": "no Context method calls it: the sliced reduce entry points, which are cases, write the same buffers",
    "ampli_event_record": EVENT, "ampli_range_event_record": EVENT,
    "ampli_graph_begin": GRAPH, "ampli_graph_end": GRAPH, "ampli_graph_launch": GRAPH,
    "ampli_set_record_layout": SETTER, "ampli_set_tuning": SETTER, "ampli_set_reduce_compact": SETTER, "ampli_set_slice_format": SETTER,
    "ampli_set_poisson_tuning": SETTER, "ampli_set_queue_items": SETTER, "ampli_set_slice_group": SETTER,
    "ampli_last_reduce_kernel": GETTER, "ampli_ranges_concurrent": GETTER, "ampli_last_spectrum_segments": GETTER,
    "ampli_comm_create": COMM,
}


# methods that are cases although api.py does not wrap them: they touch no tensor, and the case is about what the library does on the stream
EXEMPT_OR_PLAIN_IN_CASES = {"flags", "limit_stats", "power_stats", "wait_calls", "set_async_drain", "set_ranges", "ranges_join", "n_calls_total",
                            "fdr_workspace_bytes"}
# entry points a case calls on its way (through _check, or to set up what it is about) without being about them
CALLED_ON_THE_WAY = {"ampli_last_error", "ampli_set_ranges", "ampli_set_async_drain"}


def _header_path():
    import os

    from amplisolve_amd import _lib

    return os.path.join(_lib.INCLUDE, "amplisolve_hip.h")


def ctx_prototypes():
    """the ampli_* prototypes of include/amplisolve_hip.h whose first parameter is an ampli_ctx *: read by the Reader of
    amplisolve_amd/_headers.py itself, which is asked to remember how every function's first parameter is spelt"""
    from amplisolve_amd import _lib
    from amplisolve_amd._headers import Reader

    class Spellings(Reader):
        first = {}

        def declared(self, decl, where):
            if where.endswith(": parameter"):
                self.first.setdefault(where[:-len(": parameter")], decl.strip())
            return super().declared(decl, where)

    r = Spellings(types={"ampli_host_chunk_fn": _lib.CHUNK_FN, "ampli_host_shard": _lib.HostShard}, data=("ampli_call", "ampli_loo_call", "ampli_dilute_mix"))
    r.read(_lib._header("amplisolve_types.h"))
    protos = r.read(_lib._header("amplisolve_hip.h"))
    assert set(protos) == set(_lib.HIP_SYMBOLS), "the bindings were read from other prototypes"
    return [n for n in protos if re.match(r"(const\s+)?ampli_ctx\s*\*", r.first.get(n, ""))]
