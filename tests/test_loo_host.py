"""The leave-one-out mode without a GPU: its export and list entry, and the exactness argument it rests on on the CPU
oracle -- inside the envelope the S-1 sums are the whole cohort's minus the held-out normal's own addends, bit for bit."""
import ctypes as C

import numpy as np

from amplisolve_amd import _lib
from oracle import pyoracle as orc
from tests.helpers import edge_case_recs, synth_recs

ABSENT = np.iinfo(np.int32).min


def test_loo_export_and_list_entry():
    lib = C.CDLL(_lib.HIP_LIB_PATH)
    assert hasattr(lib, "ampli_loo_call_records")
    assert C.sizeof(_lib.LooCall) == C.sizeof(_lib.Call) + 16 == 80
    assert _lib.LooCall.thr_fw.offset == 64


def _own_addends(rec, C_value, cov):
    """snt / srd / cnt contributions of one record (EE:1595-1606) in the reference's operation order, as the kernel takes them out"""
    fw, bw = rec[:4].astype(np.int64), rec[4:].astype(np.int64)
    FW, BW = int(fw.sum()), int(bw.sum())
    out = []
    if rec[0] == ABSENT or FW < cov or BW < cov:
        return FW, BW, out
    for nt in range(4):
        if orc.lib().oracle_af_gate(int(fw[nt]), FW) and orc.lib().oracle_af_gate(int(bw[nt]), BW):
            out.append(nt)
    return FW, BW, out


def test_totals_minus_one_normal_are_the_s_minus_1_sums():
    rng = np.random.default_rng(7)
    P, S = 200, 9
    recs = synth_recs(P, S)
    recs[:, :40] = edge_case_recs(40, S, rng)
    for C_value, cov in ((0.002, 100), (0.001, 30), (0.004, 1)):
        tot = orc.error_reduce(recs, P, C_value, cov)
        assert tot["order_sensitive"] == 0
        for s in range(S):
            sub = orc.error_reduce(np.delete(recs, s, axis=0), P, C_value, cov)
            snt, srd, cnt = tot["snt"].copy(), tot["srd"].copy(), tot["cnt"].copy()
            for p in range(P):
                FW, BW, qual = _own_addends(recs[s, p], C_value, cov)
                pf, pb = float(np.float32(np.float32(FW) * np.float32(C_value))), float(np.float32(np.float32(BW) * np.float32(C_value)))
                for nt in qual:
                    snt[0, nt, p] = snt[0, nt, p] - float(recs[s, p, nt]) - pf
                    snt[1, nt, p] = snt[1, nt, p] - float(recs[s, p, 4 + nt]) - pb
                    srd[0, nt, p] -= FW
                    srd[1, nt, p] -= BW
                    cnt[nt, p] -= 1
            assert np.array_equal(snt.view(np.int64), sub["snt"].view(np.int64))
            assert np.array_equal(srd, sub["srd"]) and np.array_equal(cnt, sub["cnt"])
            assert np.array_equal(tot["nrec"] - (recs[s, :, 0] != ABSENT), sub["nrec"])
