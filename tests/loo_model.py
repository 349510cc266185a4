"""The leave-one-out check of a panel of normals composed from the CPU oracle's existing pieces -- TEST INFRASTRUCTURE.

For every normal s: the error table of the other S-1 normals (orc.error_reduce + orc.error_finalize over the cohort without s),
then the calling gate on s alone against that table (orc.poisson_call with the calling cut-off).  This is what the reference does
in two runs per normal (AmpliSolveErrorEstimation over S-1 files, AmpliSolveVariantCalling over s's file), and what
ampli_loo_call_records must equal bit for bit.
"""
from __future__ import annotations

import numpy as np

from oracle import pyoracle as orc

ABSENT = np.iinfo(np.int32).min


def callable_records(recs, ref_code, call_cov, ext_pos=None):
    """bool [S][R]: present, reference base in ACGT, FW >= and BW >= call_cov (VC:898, VC:3290)"""
    recs = np.asarray(recs, np.int64)
    P = ref_code.shape[0]
    R = recs.shape[1]
    pos = np.arange(R)
    if R > P:
        pos[P:] = ext_pos
    present = recs[:, :, 0] != ABSENT
    fw = recs[:, :, 0:4].sum(axis=2)
    bw = recs[:, :, 4:8].sum(axis=2)
    return present & (ref_code[pos] <= 3)[None, :] & (fw >= call_cov) & (bw >= call_cov)


def loo_model(recs, P, ref_code, C_value, cov, call_cov, E=0, dup_off=None, ext_pos=None, rd=None):
    """recs int32 [S][P+E][8] (the dense interchange layout), rd optional int32 [S][P+E] (INT32_MIN where the line is regular).
    Returns call_mask [S][R] uint8, q [S][R][4][2] (the reference's dense scores), thr_loo [S][2][4][P] float32, callable_pos [P],
    callable_sample [S] and order_sensitive (the whole cohort's totals are outside the exactness envelope)."""
    recs = np.ascontiguousarray(recs, np.int32)
    ref_code = np.ascontiguousarray(ref_code, np.uint8)
    S, R = recs.shape[0], recs.shape[1]
    assert R == P + E
    mask = np.zeros((S, R), np.uint8)
    q = np.zeros((S, R, 4, 2), np.float64)
    thr_loo = np.zeros((S, 2, 4, P), np.float32)
    for s in range(S):
        keep = np.arange(S) != s
        if S > 1:
            acc = orc.error_reduce(recs[keep], P, C_value, cov, E=E, dup_off=dup_off, rd=None if rd is None else rd[keep])
            thr = orc.error_finalize(acc)["thr"]
        else:  # an empty table: no estimate anywhere, 0.01 in every cell (EE:2680-2684)
            thr = np.full((2, 4, P), 0.01, np.float32)
        res = orc.poisson_call(recs[s:s + 1], P, thr, ref_code, call_cov, E=E, ext_pos=ext_pos, dense=True,
                               rd=None if rd is None else rd[s:s + 1])
        mask[s] = res["call_mask"][0]
        q[s] = res["q"][0]
        thr_loo[s] = thr
    live = callable_records(recs, ref_code, call_cov, ext_pos)
    pos = np.arange(R)
    if E:
        pos[P:] = ext_pos
    callable_pos = np.bincount(pos, weights=live.sum(axis=0), minlength=P).astype(np.int32)
    order_sensitive = orc.error_reduce(recs, P, C_value, cov, E=E, dup_off=dup_off, rd=rd)["order_sensitive"]
    return dict(call_mask=mask, q=q, thr_loo=thr_loo, callable_pos=callable_pos, callable_sample=live.sum(axis=1).astype(np.int32),
                order_sensitive=order_sensitive)
