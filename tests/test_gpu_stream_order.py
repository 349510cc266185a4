"""Every device-working Context method held to its context's stream (the harness and the cases: tests/stream_order.py).

The context is created under torch.cuda.stream(S) and every method is called from outside that block, in two modes that turn a
misplaced operation into a wrong answer: "S delayed" (the inputs hold a decoy and the outputs the sentinel until copies behind a delay
on S put the real inputs there) and "other stream delayed" (the caller's current stream is busy, both allocator pools hold sentinel
blocks, the method allocates and uploads for itself).  Four wrong wrappers of one small method -- a zero fill, an upload, a readback on
the other stream, the kernel launched through a second context there -- show that each mode flags what it is built for.

Methods that synchronise the stream by contract skip the not-complete assertion of "S delayed", and only that:
  flags        include/amplisolve_hip.h, ampli_ctx_flags: "Flags raised by kernels of this context since the last clear (synchronises the stream)."
  limit_stats  ampli_limit_stats: "... reset != 0 clears them.  Synchronises the stream."
  power_stats  ampli_power_stats: "... reset != 0 clears them.  Synchronises the stream."
  acc_merge    ampli_acc_merge: "Synchronises the stream: the list of the parts' pointers is uploaded from the caller's stack."
  pack16, pack24, read_calls (with n_calls_total), read_loo_calls: they return host values -- Context: "A method that returns host values
  ... synchronises that stream and no other."
"""
import contextlib

import numpy as np
import pytest

from tests import stream_order as so

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in so.cases()]


@pytest.fixture(scope="module")
def env(ctx):
    e = so.Env()
    print(f"stream order: {e.cycles_per_ms:.0f} cycles of torch.cuda._sleep per ms; the other stream is {'the default stream' if e.other_is_default else 'a created stream D'}; "
          f"probes (other, candidate, overlaps both ways, so do its two ranges' streams): {e.tried}")
    yield e
    e.close()
    waits = {c.name for c in so.cases() if c.syncs} | {"small_pack16"}
    took = {k: v for k, v in so.ENQUEUE_MS.items() if not (k[1] == "s_delayed" and k[0] in waits) and k[0] != "small_pack16"}  # (those wait for the delay itself)
    if took:
        worst = max(took, key=took.get)
        print(f"stream order: the longest host enqueue was {took[worst]:.2f} ms ({worst}); the delay is {so.DELAY_MS} ms")


@pytest.fixture(scope="module")
def world(ctx):
    return so.World(ctx)


def test_no_delay_is_longer_than_500_ms():
    """(that the delay outlasts a case's enqueue is asserted by every case: the delay must still run when everything is enqueued; how
    many times longer it is -- five, when DELAY_MS was set -- is printed when the module ends)"""
    assert so.DELAY_MS <= so.MAX_DELAY_MS and so.PROBE_MS <= so.DELAY_MS


@pytest.mark.parametrize("name", NAMES)
def test_s_delayed(ctx, env, world, name):
    env.require()
    case = so.case(name)
    want = so.expected(ctx, case, world)
    bad = so.s_delayed(env, case, world, want)
    print(f"{name}: enqueue {so.ENQUEUE_MS[name, 's_delayed']:.3f} ms")
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_other_stream_delayed(ctx, env, world, name):
    env.require()
    case = so.case(name)
    want = so.expected(ctx, case, world)
    bad = so.other_delayed(env, case, world, want)
    print(f"{name}: enqueue {so.ENQUEUE_MS[name, 'other_delayed']:.3f} ms")
    assert not bad, bad


# ---- the harness proves itself: wrong wrappers of one small method (pack16 as api.py has it, spelt out) ----------------------------

def small_pack16(env, wrong=None):
    """Context.pack16 over a host array or a device tensor: (int16 records, fits).  wrong: "fill" / "upload" / "readback": that one
    operation on the caller's current stream instead of the context's; "kernel": the launch through a second context on that stream.
    All of them race on valid, in-bounds buffers: wrong numbers, never a fault."""
    def call(ctx, x, o):
        import torch

        other = torch.cuda.current_stream()

        def place(what):
            return torch.cuda.stream(other) if wrong == what else contextlib.nullcontext()

        with torch.cuda.stream(ctx.stream):
            recs = x["over"]
            if isinstance(recs, np.ndarray):
                with place("upload"):
                    recs = torch.from_numpy(recs).to(ctx.device)
            out = torch.empty(recs.shape, dtype=torch.int16, device=ctx.device)
            with place("fill"):
                over = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
            k = env.ctx_other if wrong == "kernel" else ctx
            k._check(k.lib.ampli_records_pack16(k.h, recs.data_ptr(), recs.numel() // 8, out.data_ptr(), over.data_ptr()))
            with place("readback"):
                fits = int(over.item()) == 0
        return dict(out=out, fits=fits)

    return call


SMALL = so.Case("small_pack16", (), lambda w, v: dict(over=w.get("core", v)["over_b"]), None, host_ok=("over",), syncs=so.SYNC_HOST)
FLAGGED_BY = {"fill": so.other_delayed, "upload": so.other_delayed, "readback": so.s_delayed, "kernel": so.s_delayed}


def test_the_small_method_spelt_out_passes_both_modes(ctx, env, world):
    env.require()
    SMALL.call = small_pack16(env)
    want = so.expected(ctx, SMALL, world)
    assert so.s_delayed(env, SMALL, world, want) == [] and so.other_delayed(env, SMALL, world, want) == []


@pytest.mark.parametrize("wrong", sorted(FLAGGED_BY))
def test_a_wrong_wrapper_is_flagged_by_the_mode_built_for_it(ctx, env, world, wrong):
    env.require()
    SMALL.call = small_pack16(env)
    want = so.expected(ctx, SMALL, world)
    bad = FLAGGED_BY[wrong](env, SMALL, world, want, call=small_pack16(env, wrong))
    print(f"{wrong}: {bad}")
    assert bad, f"a {wrong} on the other stream went unnoticed"


# ---- the levels of detection_limits / detection_power: uploaded once per distinct set -----------------------------------------------

def test_levels_are_kept_per_set_and_a_full_store_is_emptied(ctx, world):
    """detection_limits keeps the device copy of every distinct set of levels (an upload per call would wait for the stream): a second
    set gets its own counts, a set gives the same counts before and after 64 other sets have emptied the store, and the store never
    holds more than 64."""
    from tests.stream_order import _dev, _host

    d = world.get("wide", "A")
    P, N = d["meta"]["P"], d["meta"]["N"]
    rec = ctx.records(_dev(d["recs"]), "i32", N)
    thr, ref = _dev(d["thr"]), _dev(d["ref"])

    def counts(levels):
        return _host(ctx.detection_limits(rec, P, thr, ref, 100, levels)["counts"])

    a, b = counts((0.005, 0.02)), counts((0.5, 0.02))
    assert a.shape == b.shape and np.array_equal(a[:, -1], b[:, -1]) and not np.array_equal(a[:, -2], b[:, -2])  # the level in common, the one that differs
    for i in range(70):
        one = counts((0.001 + i * 1e-4,))
        assert one.shape[1] == a.shape[1] - 1 and len(ctx._level_sets) <= 64
    assert (0.005, 0.02) not in ctx._level_sets
    assert np.array_equal(counts((0.005, 0.02)), a) and np.array_equal(counts((0.5, 0.02)), b)
