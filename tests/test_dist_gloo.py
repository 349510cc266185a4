"""The multi-rank merge protocol (amplisolve_amd/dist.py) over gloo, world_size 2, 3 and 8 (the node's rank count: 23 samples and 1500
positions divide by neither), on CPU.

Each rank reduces its contiguous shard of the normal samples (here with the oracle, since there is no GPU),
then the ranks merge exactly as bench.py does over RCCL: all-reduce SUM of the additive planes, all-gather
of the germ-max regions, ordered fold.  Result must equal the single-pass table bit for bit on every rank."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from amplisolve_amd.api import Acc
from amplisolve_amd.dist import SlicedMerger, TableMerger, merge_error_table, shard_range, slice_geometry, table_regions
from oracle import pyoracle as orc
from tests.helpers import synth_recs

P, S = 1500, 23


def host_fold(acc, gathered, world):
    """numpy twin of ampli_gm_merge (csrc/ampli_exchange.hip gm_merge_kernel)."""
    _, gm_off, gm_bytes = table_regions(acc.P)
    n4 = 4 * acc.P
    offs = [0, None, acc.struct.gm_first_af - acc.struct.gm_n, acc.struct.gm_rest - acc.struct.gm_n]  # gm_first is not exchanged
    g = gathered.numpy().reshape(world, gm_bytes)
    n = np.zeros(n4, np.int32); first = np.full(n4, 0x7fffffff, np.int32)
    faf = np.zeros(n4, np.float32); rest = np.full(n4, -np.inf, np.float32)
    for k in range(world):
        rn = g[k, offs[0]: offs[0] + 4 * n4].view(np.int32)
        rf = np.full(n4, -1, np.int32)
        ra = g[k, offs[2]: offs[2] + 4 * n4].view(np.float32)
        rr = g[k, offs[3]: offs[3] + 4 * n4].view(np.float32)
        has, empty = rn > 0, n == 0
        take = has & empty
        first[take], faf[take], rest[take] = rf[take], ra[take], rr[take]
        fold = has & ~empty
        rest[fold] = np.maximum(rest[fold], np.maximum(ra[fold], rr[fold]))
        n = n + rn
    acc.gm_n.copy_(torch.from_numpy(n.reshape(4, acc.P)))
    acc.gm_first.copy_(torch.from_numpy(first.reshape(4, acc.P)))
    acc.gm_first_af.copy_(torch.from_numpy(faf.reshape(4, acc.P)))
    acc.gm_rest.copy_(torch.from_numpy(rest.reshape(4, acc.P)))


def worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        recs = synth_recs(P, S)
        lo, hi = shard_range(S, rank, world)
        part = orc.error_reduce(recs[lo:hi], P, 0.002, 100, first_sample=lo)
        acc = Acc(None, P, device="cpu")
        acc.buf.zero_()
        for name in ("snt", "srd", "cnt", "nrec", "gm_n", "gm_first", "gm_first_af", "gm_rest"):
            getattr(acc, name).copy_(torch.from_numpy(part[name]))
        merge_error_table(acc, host_fold)
        full = orc.error_reduce(recs, P, 0.002, 100)
        ok = True
        for name in ("snt", "srd", "cnt", "nrec", "gm_n"):
            ok &= bool(np.array_equal(getattr(acc, name).numpy(), full[name]))
        m1, m2 = full["gm_n"] > 0, full["gm_n"] > 1
        ok &= bool(np.array_equal(acc.gm_first_af.numpy()[m1].view(np.int32), full["gm_first_af"][m1].view(np.int32)))
        ok &= bool(np.array_equal(acc.gm_rest.numpy()[m2].view(np.int32), full["gm_rest"][m2].view(np.int32)))
        # the pipelined, double-buffered form bench.py uses at N > 1: two batches in flight
        merger = TableMerger(P, world, "cpu", host_fold)
        batches = []
        for b in range(2):
            rb = synth_recs(P, S, seed=1234 + b)
            pb = orc.error_reduce(rb[lo:hi], P, 0.002, 100, first_sample=lo)
            ab = Acc(None, P, device="cpu")
            ab.buf.zero_()
            for name in ("snt", "srd", "cnt", "nrec", "gm_n", "gm_first", "gm_first_af", "gm_rest"):
                getattr(ab, name).copy_(torch.from_numpy(pb[name]))
            batches.append((rb, ab, merger.start(ab, b)))
        for b, (rb, ab, h) in enumerate(batches):
            merger.finish(ab, b, h)
            fb = orc.error_reduce(rb, P, 0.002, 100)
            for name in ("snt", "srd", "cnt", "nrec", "gm_n"):
                ok &= bool(np.array_equal(getattr(ab, name).numpy(), fb[name]))
            mb = fb["gm_n"] > 1
            ok &= bool(np.array_equal(ab.gm_rest.numpy()[mb].view(np.int32), fb["gm_rest"][mb].view(np.int32)))
        fin_a = orc.error_finalize({k: getattr(acc, k).numpy() for k in ("snt", "srd", "cnt", "nrec", "gm_n", "gm_rest")})
        fin_b = orc.error_finalize(full)
        ok &= all(np.array_equal(fin_a[k], fin_b[k], equal_nan=True) for k in fin_a)
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


# ---- position-sliced merge: numpy twins of the three kernels around SlicedMerger's collectives ----
def host_pack_sliced(part, P, world, L, sums, gm, slim=False):
    """twin of lane_acc_store_sliced (csrc/ampli_kernels.hip): partial table -> slice-major exchange buffers.
    slim: 14 planes -- the two strands' depth sums of a nucleotide as lo + hi * 2^26, the counts three to a double in base 2^17"""
    srd, cnt, nrec = part["srd"].astype(np.float64), part["cnt"].astype(np.float64), part["nrec"].astype(np.float64)
    if slim:
        assert (part["srd"] < (1 << 26) // world).all() and (part["cnt"] < (1 << 17) // world).all() and (part["nrec"] < (1 << 17) // world).all()
        planes = np.concatenate([part["snt"].reshape(8, P), srd[0] + srd[1] * 2.0 ** 26,
                                 (cnt[0] + cnt[1] * 2.0 ** 17 + cnt[2] * 2.0 ** 34).reshape(1, P), (cnt[3] + nrec * 2.0 ** 17).reshape(1, P)])
    else:
        planes = np.concatenate([part["snt"].reshape(8, P), srd.reshape(8, P), cnt, nrec.reshape(1, P)])
    pair = np.concatenate([np.where(part["gm_n"] > 0, part["gm_first_af"], np.float32(-1)),
                           np.where(part["gm_n"] > 1, part["gm_rest"], np.float32(-np.inf))]).astype(np.float32)
    s, g = sums.numpy().reshape(world, 14 if slim else 21, L), gm.numpy().reshape(world, 8, L)
    for k in range(world):
        lo, hi = k * L, min(P, (k + 1) * L)
        if hi > lo:
            s[k, :, : hi - lo] = planes[:, lo:hi]
            g[k, :, : hi - lo] = pair[:, lo:hi]


def host_finalize_slice(sum_slice, gm_recv, world, L, n_valid, slim=False):
    """twin of error_finalize_slice_kernel: ordered fold of the shards' germ-max pairs + the oracle's finalize."""
    s, g = sum_slice.numpy().reshape(14 if slim else 21, L)[:, :n_valid], gm_recv.numpy().reshape(world, 8, L)[:, :, :n_valid]
    if slim:  # the summed fields come apart again
        hi = np.floor(s[8:12] / 2.0 ** 26)
        c2 = np.floor(s[12] / 2.0 ** 34)
        r = s[12] - c2 * 2.0 ** 34
        c1 = np.floor(r / 2.0 ** 17)
        n1 = np.floor(s[13] / 2.0 ** 17)
        s = np.concatenate([s[:8], s[8:12] - hi * 2.0 ** 26, hi, np.stack([r - c1 * 2.0 ** 17, c1, c2, s[13] - n1 * 2.0 ** 17]), n1.reshape(1, -1)])
    n = np.zeros((4, n_valid), np.int32)
    rest = np.full((4, n_valid), -np.inf, np.float32)
    for k in range(world):
        fa, rr = g[k, :4], g[k, 4:]
        has = fa >= 0
        first = has & (n == 0)
        later = has & (n > 0)
        rest[later] = np.maximum(rest[later], np.maximum(fa[later], rr[later]))
        n[later] = 2
        rest[first] = rr[first]
        n[first] = np.where(rr[first] > -np.inf, 2, 1)
    acc = dict(snt=np.ascontiguousarray(s[:8].reshape(2, 4, n_valid)), srd=np.ascontiguousarray(s[8:16].reshape(2, 4, n_valid).astype(np.int64)),
               cnt=np.ascontiguousarray(s[16:20].astype(np.int32)), nrec=np.ascontiguousarray(s[20].astype(np.int32)),
               gm_n=n, gm_rest=rest)
    return orc.error_finalize(acc)


def sliced_worker(rank, world, port, q, slim=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        L, _, _, block_bytes = slice_geometry(P, world, slim)
        merger = SlicedMerger(P, world, rank, "cpu", slim=slim)
        assert merger.planes == (14 if slim else 21) and merger.bytes_received_per_step()["reduce_scatter_f64"] == (world - 1) * merger.planes * L * 8
        lo, hi = shard_range(S, rank, world)
        n_valid = max(0, min(P, (rank + 1) * L) - rank * L)
        ok = True
        batches = []
        for b in range(3):  # three batches in flight, as bench.py keeps them
            rb = synth_recs(P, S, seed=4321 + b)
            host_pack_sliced(orc.error_reduce(rb[lo:hi], P, 0.002, 100, first_sample=lo), P, world, L, merger.sums[b], merger.gm[b], slim)
            batches.append((rb, merger.start_exchange(b)))
        gathers = []
        for b, (rb, h) in enumerate(batches):
            merger.wait(h)
            fin = host_finalize_slice(merger.sum_slice[b], merger.gm_recv[b], world, L, n_valid, slim)
            # block = this rank's slice of the table, serialised (here: rate | thr | code | germ_present | germ_val as f64)
            blob = np.concatenate([fin["rate"].reshape(-1).view(np.uint8), fin["thr"].reshape(-1).view(np.uint8), fin["code"].reshape(-1),
                                   fin["germ_present"].reshape(-1), fin["germ_val"].reshape(-1).view(np.uint8)])
            assert blob.size <= block_bytes + 16 * L  # f64 germ values in the host twin; the device block carries f32
            blk = torch.zeros(104 * L, dtype=torch.uint8)
            blk[: blob.size] = torch.from_numpy(blob)
            merger.block[b] = blk
            merger.blocks[b] = torch.zeros(world * 104 * L, dtype=torch.uint8)
            gathers.append((rb, merger.start_gather(b)))
        for b, (rb, h) in enumerate(gathers):
            merger.wait(h)
            full = orc.error_finalize(orc.error_reduce(rb, P, 0.002, 100))
            allb = merger.blocks[b].numpy().reshape(world, 104 * L)
            for k in range(world):
                nv = max(0, min(P, (k + 1) * L) - k * L)
                if nv == 0:
                    continue
                sl = slice(k * L, k * L + nv)
                o = 0
                for name, shape, dt in (("rate", (2, 4, nv), np.float32), ("thr", (2, 4, nv), np.float32), ("code", (4, nv), np.uint8),
                                        ("germ_present", (4, nv), np.uint8), ("germ_val", (4, nv), np.float64)):
                    nb = int(np.prod(shape)) * np.dtype(dt).itemsize
                    got = allb[k, o:o + nb].view(dt).reshape(shape)
                    o += nb
                    exp = full[name][..., sl]
                    if name == "germ_val":
                        m = full["germ_present"][..., sl] > 0
                        ok &= bool(np.array_equal(got[m], exp[m]))
                    else:
                        ok &= bool(np.array_equal(got.view(np.uint8), np.ascontiguousarray(exp).view(np.uint8)))
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,slim", [(2, False), (2, True), (3, False), (3, True), (8, True), (8, False)])
def test_sliced_merge_protocol_over_gloo(world, slim):
    """Slice ownership, chunk order of the reduce-scatter / all-to-all / all-gather and the ordered germ-max fold:
    every rank ends with every slice of the single-pass error table, bit for bit -- with the sums as 21 plain planes and as the
    14 packed planes of the slim format (the fields of a packed double add up independently; round 4)."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=sliced_worker, args=(r, world, port, q, slim)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(60)
    assert sorted(r for r, _ in res) == list(range(world))
    assert all(ok for _, ok in res)


def test_shard_range_partitions():
    for n in (1, 7, 96, 1024):
        for w in (1, 2, 3, 8):
            cuts = [shard_range(n, r, w) for r in range(w)]
            assert cuts[0][0] == 0 and cuts[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
            assert max(b - a for a, b in cuts) - min(b - a for a, b in cuts) <= 1


@pytest.mark.parametrize("world", [2, 3, 8])
def test_merge_protocol_over_gloo(world):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(60)
    assert sorted(r for r, _ in res) == list(range(world))
    assert all(ok for _, ok in res)
