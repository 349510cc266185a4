"""The definition of the in-silico dilution -- TEST INFRASTRUCTURE, and the text that include/amplisolve_hip.h,
csrc/ampli_math.h and DESIGN 22 restate.  Read-level mixing of two count files: 32-bit integer work only, so the device, the host
library and this model agree integer for integer.

  Generator.  Philox4x32-10 (Salmon et al., 2011).  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments W0 = 0x9E3779B9,
    W1 = 0xBB67AE85.  One round on counter (c0, c1, c2, c3) with key (k0, k1): (hi0, lo0) = M0 * c0 as a 64-bit product,
    (hi1, lo1) = M1 * c2; the new counter is (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0).  Ten rounds; the key is bumped by (W0, W1)
    after each round (the bump after the last round is dead).
  Thinning.  Thin(n, keep; key, p, f, side) = #{ i < n : word_i < keep }, compared as 64-bit unsigned, keep in [0, 2^32].  word_i is
    output word (i & 3) of Philox with counter (i >> 2, p, f | side << 3, 0) and key (low word, high word of the 64-bit key); p is the
    position index, f in 0..7 the record field, side 0 for file a and 1 for file b.  A read is word i of its field, kept with
    probability keep / 2^32, independently.  Exactly: keep = 2^32 keeps all, keep = 0 keeps none, Thin is non-decreasing in n and in
    keep -- so a series with one key is nested.
  Mixture.  {int32 row_a; int32 row_b; uint64 keep_a; uint64 keep_b; uint64 key}: out[f] = Thin(a[f], keep_a; key, p, f, 0) +
    Thin(b[f], keep_b; key, p, f, 1) over the PRIMARY records; row_b == -1 is pure down-sampling.  The output record is ABSENT
    (field 0 = AMPLI_ABSENT, the other seven 0) when a's record is absent, when b is named and its record is absent, or when a present
    input record holds a count outside [0, 2^24 - 2] (AMPLI_DILUTE_BAD_COUNT).  A mixture is all ABSENT with AMPLI_DILUTE_BAD_MIXTURE
    when a row is outside its chunk, a keep is above 2^32, row_b >= 0 without a chunk b, or row_b < -1.
  Fractions to thresholds.  keep = (uint64) floor(ldexp(x, 32) + 0.5), x a double in [0, 1]: IEEE operations, the same everywhere.

This model draws every word, also where keep is 0 or 2^32: the identities the kernel and the host library use as shortcuts are
consequences here, not rules."""
import math

import numpy as np

ABSENT = np.iinfo(np.int32).min
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KEEP_ALL = 1 << 32
MAX_COUNT = (1 << 24) - 2
BAD_COUNT, BAD_MIXTURE = 1, 2
MASK = np.uint64(0xFFFFFFFF)
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of arrays (or scalars) of counter and key words; four uint64 arrays holding 32-bit words"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # a 32 x 32 bit product fits 64 bits
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def keep_of(x):
    """the threshold of a fraction x in [0, 1]"""
    assert 0.0 <= x <= 1.0
    return int(math.floor(math.ldexp(float(x), 32) + 0.5))


def thin_cells(n, keep, key, p, fs, chunk=1 << 22):
    """Thin of many cells at once: n, keep, key, p, fs (= f | side << 3) are arrays of one length or scalars (keep and key as
    unsigned 64-bit values); every cell has 0 <= n.  Returns int64 kept counts."""
    n = np.asarray(n, dtype=np.int64)
    C = len(n)
    keep = np.broadcast_to(np.asarray(keep, dtype=np.uint64), (C,))
    key = np.broadcast_to(np.asarray(key, dtype=np.uint64), (C,))
    p = np.broadcast_to(np.asarray(p, dtype=np.uint64), (C,))
    fs = np.broadcast_to(np.asarray(fs, dtype=np.uint64), (C,))
    assert (n >= 0).all()
    blocks = (n + 3) // 4
    out = np.zeros(C, np.int64)
    first = np.concatenate([[0], np.cumsum(blocks)])
    total = int(first[-1])
    for lo in range(0, total, chunk):  # the flat list of blocks, a slice at a time
        hi = min(total, lo + chunk)
        g = np.arange(lo, hi, dtype=np.int64)
        cell = np.searchsorted(first, g, side="right") - 1
        j = g - first[cell]
        w = philox(j.astype(np.uint64), p[cell], fs[cell], 0, key[cell] & MASK, key[cell] >> np.uint64(32))
        live = np.minimum(4, n[cell] - 4 * j)
        got = np.zeros(len(g), np.int64)
        for i in range(4):
            got += (i < live) & (w[i] < keep[cell])
        out += np.bincount(cell, weights=got, minlength=C).astype(np.int64)
    return out


def thin(n, keep, key, p, f, side):
    return int(thin_cells([n], keep, key, [p], [f | side << 3])[0])


def mix_ok(row_a, row_b, keep_a, keep_b, n_a, n_b, has_b):
    if row_a < 0 or row_a >= n_a or keep_a > KEEP_ALL or keep_b > KEEP_ALL or row_b < -1:
        return False
    return row_b == -1 or (has_b and row_b < n_b)


def dilute_model(recs_a, recs_b, P, mixtures):
    """recs_a int32 [n_a][>= P][8], recs_b likewise or None, mixtures a list of (row_a, row_b, keep_a, keep_b, key).  Returns out int32
    [n_mix][P][8] and flags int32 [n_mix].  Only the first P records of a row enter."""
    n_mix = len(mixtures)
    out = np.zeros((n_mix, P, 8), np.int32)
    out[:, :, 0] = ABSENT
    flags = np.zeros(n_mix, np.int32)
    cn, ck, cy, cp, cf, dst = [], [], [], [], [], []
    pos = np.arange(P)
    for m, (row_a, row_b, keep_a, keep_b, key) in enumerate(mixtures):
        if not mix_ok(row_a, row_b, keep_a, keep_b, len(recs_a), len(recs_b) if recs_b is not None else 0, recs_b is not None):
            flags[m] = BAD_MIXTURE
            continue
        a = recs_a[row_a, :P].astype(np.int64)
        pres_a = a[:, 0] != ABSENT
        bad = pres_a & ((a < 0) | (a > MAX_COUNT)).any(-1)
        present = pres_a
        b = None
        if row_b >= 0:
            b = recs_b[row_b, :P].astype(np.int64)
            pres_b = b[:, 0] != ABSENT
            bad |= pres_b & ((b < 0) | (b > MAX_COUNT)).any(-1)
            present = present & pres_b
        if bad.any():
            flags[m] |= BAD_COUNT
        present = present & ~bad
        idx = pos[present]
        for side, r, keep in ((0, a, keep_a), (1, b, keep_b)):
            if r is None:
                continue
            for f in range(8):
                cn.append(r[idx, f]); cp.append(idx); cf.append(np.full(len(idx), f | side << 3))
                ck.append(np.full(len(idx), keep, dtype=np.uint64)); cy.append(np.full(len(idx), key & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
                dst.append((m * P + idx) * 8 + f)
        out[m, idx, 0] = 0
    if cn:
        got = thin_cells(np.concatenate(cn), np.concatenate(ck), np.concatenate(cy), np.concatenate(cp), np.concatenate(cf))
        flat = out.reshape(-1)
        np.add.at(flat, np.concatenate(dst), got.astype(np.int32))
    return out, flags


# ---- the command line (AmpliSolveInSilicoDilution, csrc/host/run_di.cpp): keys, truth cells, the three texts ---------------------------
M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def mixture_key(seed, ia, ib, rep):
    """ia, ib: the indices of the two files in the sample list's visit order, ib = -1 without a diluent; rep < 2^20"""
    return splitmix64(seed ^ splitmix64(((ia << 40) ^ ((ib + 1) << 20) ^ rep) & M64))


def called_cells(recs, thr, ref, cov):
    """the gate's bit for every (row, position, base) of primary records int32 [n][P][8]: both strands covered and Q >= 5 on both"""
    from tests.limit_model import score

    n, P = recs.shape[:2]
    out = np.zeros((n, P, 4), bool)
    for s in range(n):
        for p in range(P):
            r = recs[s, p]
            if r[0] == ABSENT or ref[p] > 3:
                continue
            FW, BW = int(r[:4].sum()), int(r[4:].sum())
            if FW < cov or BW < cov:
                continue
            for nt in range(4):
                if nt != ref[p]:
                    out[s, p, nt] = score(r[nt], FW, thr[0, nt, p]) >= 5 and score(r[4 + nt], BW, thr[1, nt, p]) >= 5
    return out


def series(names, recs, thr, ref, lines, replicates, seed, cov, conf, mix=None):
    """The dilution series of the command.  names: the files in visit order; recs int32 [F][P][8] their primary records; lines:
    (source, diluent or "-", fraction, scale).  mix(recs_a, recs_b, P, mixtures) -> (out, flags) does the mixing (default: dilute_model;
    the command's test passes the host library, which tests/test_dilution_host.py holds to this model, for its speed).  Returns per
    line a dict: truth [(p, nt)], v_exp, detected, predicted (summed over the replicates), novel [replicates], depth sums, present,
    flagged, out int32 [replicates][P][8]."""
    import ctypes as C

    from amplisolve_amd import host_lib
    from tests.limit_model import OK, pair_limit

    H = host_lib()
    mix = mix or dilute_model
    P = recs.shape[1]
    index = {n: i for i, n in enumerate(names)}
    base = called_cells(recs, thr, ref, cov)
    res = []
    for src, dil, fraction, scale in lines:
        ia, ib = index[src], index[dil] if dil != "-" else -1
        keep_a, keep_b = keep_of(fraction * scale), keep_of((1.0 - fraction) * scale)
        ca, cb = base[ia], base[ib] if ib >= 0 else np.zeros((P, 4), bool)
        truth = [(int(p), int(nt)) for p, nt in np.argwhere(ca & ~cb)]
        v_exp = []
        for p, nt in truth:
            x = recs[ia, p].astype(np.int64)
            y = recs[ib, p].astype(np.int64) if ib >= 0 and recs[ib, p, 0] != ABSENT else np.zeros(8, np.int64)
            den = float(x.sum()) * float(keep_a) + float(y.sum()) * float(keep_b)
            v_exp.append((float(x[nt] + x[4 + nt]) * float(keep_a) + float(y[nt] + y[4 + nt]) * float(keep_b)) / den if den > 0 else 0.0)
        mixtures = [(ia, ib, keep_a, keep_b, mixture_key(seed, ia, ib, rep)) for rep in range(replicates)]
        out, flags = mix(recs, recs, P, mixtures)
        got = called_cells(out, thr, ref, cov)
        detected, predicted = [0] * len(truth), [0.0] * len(truth)
        for rep in range(replicates):
            for t, (p, nt) in enumerate(truth):
                detected[t] += bool(got[rep, p, nt])
                r = out[rep, p]
                if r[0] == ABSENT or not v_exp[t] > 0:
                    continue
                st, mf, mb, _ = pair_limit(r, int(r.astype(np.int64).sum()), nt, thr[0, nt, p], thr[1, nt, p], cov, from_one=False)
                if st == OK:
                    pw = C.c_double()
                    assert H.ampli_host_power_pair(int(r[:4].sum()), mf, int(r[4:].sum()), mb, (C.c_float * 1)(v_exp[t]), 1, C.c_float(conf), C.byref(pw), None, None) == 0
                    predicted[t] += pw.value
        present = out[:, :, 0] != ABSENT
        both = (recs[ia, :, 0] != ABSENT) & ((recs[ib, :, 0] != ABSENT) if ib >= 0 else True)
        flagged = int(((~present) & both[None, :] & (flags != 0)[:, None]).sum())
        o64 = np.where(present[:, :, None], out, 0).astype(np.int64)
        res.append(dict(line=(src, dil, fraction, scale), truth=truth, v_exp=v_exp, detected=detected, predicted=predicted,
                        novel=[int((got[rep] & ~ca & ~cb).sum()) for rep in range(replicates)], depth_fw=int(o64[:, :, :4].sum()), depth_bw=int(o64[:, :, 4:].sum()),
                        present=int(present.sum()), flagged=flagged, out=out, ia=ia))
    return res


def format_files(names, positions, ref, recs, thr, lines, replicates, seed, cov, conf, mix=None):
    """the three texts of AmpliSolveInSilicoDilution.  positions: (chrom, coordinate) per panel position.  Returns the texts by file
    name and the series (above)."""
    res = series(names, recs, thr, ref, lines, replicates, seed, cov, conf, mix)
    variants = "source\tdiluent\tfraction\tscale\tchrom\tposition\tsubstitution\tXfw\tXrs\tFW\tBW\tVAF\tv_exp\treplicates\tdetected\trate\tpredicted\n"
    per_line = "source\tdiluent\tfraction\tscale\ttruth_cells\tmean_rate\tmean_predicted\tnovel_mean\tnovel_max\tdepth_fw\tdepth_bw\tflagged_records\n"
    tot = [0, 0, 0, 0]
    for r in res:
        src, dil, fraction, scale = r["line"]
        head = f"{src}\t{dil}\t{fraction:g}\t{scale:g}"
        rates, preds = [], []
        for t, (p, nt) in enumerate(r["truth"]):
            x = recs[r["ia"], p].astype(np.int64)
            FW, BW = int(x[:4].sum()), int(x[4:].sum())
            rate, pred = r["detected"][t] / replicates, r["predicted"][t] / replicates
            rates.append(rate)
            preds.append(pred)
            vaf = float(x[nt] + x[4 + nt]) / float(FW + BW) if FW + BW else 0.0
            variants += (f"{head}\t{positions[p][0]}\t{positions[p][1]}\t{'ACGT'[ref[p]]}->{'ACGT'[nt]}\t{x[nt]}\t{x[4 + nt]}\t{FW}\t{BW}\t{vaf:.6f}\t{r['v_exp'][t]:.6f}\t"
                         f"{replicates}\t{r['detected'][t]}\t{rate:.6f}\t{pred:.6f}\n")
        n = len(r["truth"])
        mean = (lambda v: f"{sum(v) / n:.6f}") if n else (lambda v: "NA")
        dfw = r["depth_fw"] / r["present"] if r["present"] else 0.0
        dbw = r["depth_bw"] / r["present"] if r["present"] else 0.0
        per_line += f"{head}\t{n}\t{mean(rates)}\t{mean(preds)}\t{sum(r['novel']) / replicates:.6f}\t{max(r['novel'])}\t{dfw:.2f}\t{dbw:.2f}\t{r['flagged']}\n"
        tot = [tot[0] + n, tot[1] + sum(r["detected"]), tot[2] + sum(r["novel"]), tot[3] + r["flagged"]]
    summary = (f"lines={len(lines)}\nmixtures={len(lines) * replicates}\npositions={recs.shape[1]}\nreplicates={replicates}\nseed={seed}\ncoverage_cutoff={cov}\n"
               f"confidence={conf:g}\ntruth_cells={tot[0]}\ndetected={tot[1]}\nnovel={tot[2]}\nflagged_records={tot[3]}\n")
    return {"Dilution_Variants.txt": variants, "Dilution_Lines.txt": per_line, "Dilution_Summary.txt": summary}, res
