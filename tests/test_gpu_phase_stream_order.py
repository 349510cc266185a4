"""read_phase and phase_score held to the context's stream: two Case objects of tests/stream_order.py whose `call` is the
function of amplisolve_amd/phase.py instead of a Context method, run through its Env and its two modes exactly as
tests/test_gpu_stream_order.py runs the methods' cases.  The inputs are the read walks' world (one fuzz stream of 1777 reads, its mapping
qualities zeroed in the decoy); the expected values are held to the model of tests/phase_model.py before either mode runs.  The modes run
in a child process (see both_modes).  And, without a device, both functions carry api.py's wrapper."""
import functools

import numpy as np
import pytest

from tests import phase_model as ph
from tests import stream_order as so

Q = 300


@functools.lru_cache(None)
def _tables(world):
    """{variant: the model's Result of the walk world's stream}"""
    out = {}
    for v in "AB":
        d = world.get("walk", v)
        out[v] = ph.count((d["bam"], d["rec_off"].view(np.uint64)), d["keys"].view(np.uint64), d["meta"]["mbq"], d["meta"]["mrq"])
    return out


def _walk_inputs(world, v):
    d = world.get("walk", v)
    return dict(bam=d["bam"], rec_off=d["rec_off"], keys=d["keys"])


def _score_inputs(world, v):
    table = _tables(world)[v].table
    rng = np.random.default_rng(3207)
    ref = rng.integers(0, 4, size=(Q, 2))
    alt = (ref + 1 + rng.integers(0, 3, size=(Q, 2))) % 4
    busy = np.flatnonzero(_tables(world)["A"].table.sum((2, 3)).reshape(-1))  # the same cells in both variants: those A's reads fill
    return dict(table=table.astype(np.int32), pair_cell=rng.choice(busy, size=Q).astype(np.int64), pair_nt=np.stack([ref[:, 0], alt[:, 0], ref[:, 1], alt[:, 1]], 1).astype(np.int8))


def _n_keys(world):
    return len(world.get("walk", "A")["keys"])


def _given(o, *names):
    return {k: o[k] for k in names if k in o}


def _read_phase(ctx, x, o):
    from amplisolve_amd import read_phase

    t, s = read_phase(ctx, x["bam"], x["rec_off"], x["keys"], mbq=_read_phase.meta["mbq"], mrq=_read_phase.meta["mrq"], **_given(o, "table", "stats"))
    return dict(table=t, stats=s)


def _phase_score(ctx, x, o):
    from amplisolve_amd import phase_score

    i, s, c = phase_score(ctx, x["table"], x["pair_cell"], x["pair_nt"], 1, 0, **_given(o, "ints", "score", "cls"))
    return dict(ints=i, score=s, cls=c)


def _count_model(a):
    r = ph.count((a["bam"], a["rec_off"].view(np.uint64)), a["keys"].view(np.uint64), _read_phase.meta["mbq"], _read_phase.meta["mrq"])
    return dict(table=r.table.astype(np.int32), stats=np.asarray(r.stats, np.int64))


def _score_model(a):
    s = ph.score(a["table"], a["pair_cell"], a["pair_nt"], 1, 0)
    return dict(ints=s.ints, cls=s.cls.astype(np.int32))


CASES = {
    "read_phase": so.Case("read_phase", (), _walk_inputs, _read_phase,
                          lambda w: dict(table=((_n_keys(w), ph.K, ph.STATES, ph.STATES), np.int32, "add"), stats=((3,), np.int64, "add")),
                          protos=("ampli_pileup_phase",), model=_count_model),
    "phase_score": so.Case("phase_score", (), _score_inputs, _phase_score,
                           lambda w: dict(ints=((Q, 6), np.int64, "over"), score=((Q,), np.float32, "over"), cls=((Q,), np.int32, "over")),
                           protos=("ampli_phase_score",), model=_score_model),
}


def test_both_functions_carry_the_wrapper_of_the_contexts_stream():
    from amplisolve_amd import phase, phase_score, read_phase

    assert read_phase is phase.read_phase and phase_score is phase.phase_score
    assert getattr(read_phase, "on_stream", False) is True and getattr(phase_score, "on_stream", False) is True
    assert all(c.methods == () and c.entry_points() == set(c.protos) for c in CASES.values())
    protos = so.ctx_prototypes()
    assert "ampli_pileup_phase" not in protos and "ampli_phase_score" not in protos  # the context is their LAST parameter


def run_both_modes():
    """both cases through Env, s_delayed() and other_delayed() exactly as tests/test_gpu_stream_order.py runs its own: {"case/mode": [differences]}"""
    from amplisolve_amd import Context

    ctx = Context(0)  # the session's default-stream context: the reference values come from it
    env = so.Env()
    out = {}
    try:
        env.require()
        world = so.World(ctx)
        _read_phase.meta = so._meta(world, "walk")
        for name, case in sorted(CASES.items()):
            want = so.expected(ctx, case, world)  # held to the model inside
            assert any(w.any() for w in want.values()), name
            out[f"{name}/s_delayed"] = so.s_delayed(env, case, world, want)
            out[f"{name}/other_delayed"] = so.other_delayed(env, case, world, want)
            out[f"{name}/enqueue_ms"] = [so.ENQUEUE_MS[name, "s_delayed"], so.ENQUEUE_MS[name, "other_delayed"]]
    finally:
        env.close()
        ctx.close()
    return out


@pytest.fixture(scope="module")
def both_modes():
    """The two modes in a process of their own: Env creates contexts and streams by the dozen, and how many streams a process has created
    so far decides which hardware queue the next one lands on -- the session's process, in which tests/test_gpu_stream_order.py builds
    its own Env later, creates none for this module."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_phase_stream_order"], cwd=root, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["s_delayed", "other_delayed"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_function_holds_the_stream_contract(both_modes, name, mode):
    print(f"{name}: enqueue (s_delayed, other_delayed) {both_modes[name + '/enqueue_ms']} ms")
    assert both_modes[f"{name}/{mode}"] == [], both_modes[f"{name}/{mode}"]


if __name__ == "__main__":
    import json

    print(json.dumps(run_both_modes()))
