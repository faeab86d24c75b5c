"""Host-side checks of the label-confidence outputs (lseg_forward_labels_conf / lseg_op_corr_argmax_conf, csrc/corr_argmax.hip CONF):
a numpy model of the rule the streamed kernel and its merge implement -- an online top-2 + log-sum-exp over the labels in ascending
order, in panels of 48, the panels dealt to parts that are merged in ascending order -- against the direct stable sort / logsumexp, on
inputs with forced ties; and the new entries in the header and the ctypes table."""
import os
import re

import numpy as np
import pytest

from lseg_hip import _lib

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANEL = 48


def _push(v, k, st):
    """one value into the running state [best, arg, second, arg2] (top2_push of corr_argmax.hip): strict `>` twice"""
    if v > st[0]:
        st[2], st[3] = st[0], st[1]
        st[0], st[1] = v, k
    elif v > st[2]:
        st[2], st[3] = v, k


def _part(vals, k_lo, k_hi):
    """what one workgroup keeps for labels [k_lo, k_hi): top-2 and (best, sum of exp(v - best)) with one exp per value"""
    st = [-np.inf, 0, -np.inf, 0]
    s = 0.0
    for pb in range(k_lo, k_hi, PANEL):
        for k in range(pb, min(pb + PANEL, k_hi)):
            v = vals[k]
            e = np.exp(-abs(v - st[0])) if np.isfinite(st[0]) else 0.0
            s = s * e + 1.0 if v > st[0] else s + e
            _push(v, k, st)
    label2 = -1 if st[2] == -np.inf else st[3]
    return st[0], st[1], st[2], label2, st[0] + np.log(s)


def _model(vals, nsplit):
    K = len(vals)
    panels = (K + PANEL - 1) // PANEL
    per = (panels + nsplit - 1) // nsplit
    assert per * (nsplit - 1) < panels, "the launcher never leaves the last part empty"
    parts = [_part(vals, s * per * PANEL, min((s + 1) * per * PANEL, K)) for s in range(nsplit)]
    m, a, m2, a2, l = parts[0]
    st = [m, a, m2, a2]
    for pm, pa, pm2, pa2, pl in parts[1:]:                # corr_argmax_conf_merge_kernel
        _push(pm, pa, st)
        _push(pm2, pa2, st)
        l = max(l, pl) + np.log1p(np.exp(-abs(l - pl)))
    return st[0], st[1], st[2], st[3], l


def _direct(vals):
    order = np.argsort(-vals, kind="stable")
    m = vals.max()
    lse = m + np.log(np.exp(vals - m).sum())
    if len(vals) == 1:
        return vals[order[0]], order[0], -np.inf, -1, lse
    return vals[order[0]], order[0], vals[order[1]], order[1], lse


def _cases():
    rng = np.random.default_rng(0)
    out = []
    for K, nsplit in ((1, 1), (2, 1), (47, 1), (48, 1), (49, 2), (157, 2), (300, 1), (300, 3), (300, 7), (1000, 7)):     # (21 panels over 8 parts would leave the last one empty)
        panels = (K + PANEL - 1) // PANEL
        per = (panels + nsplit - 1) // nsplit
        edge = per * PANEL                                 # first label of part 1 (= a panel boundary too)
        for trial in range(6):
            v = rng.standard_normal(K) * 3.0
            top = v.max() + 1.0
            if K >= 2 and trial == 1:                      # the maximum twice inside one panel
                v[[0, min(5, K - 1)]] = top
            if K > PANEL and trial == 2:                   # ... across a panel boundary
                v[[PANEL - 1, PANEL]] = top
            if nsplit > 1 and trial == 3:                  # ... across a part boundary, and a tied runner-up pair across it as well
                v[[edge - 1, edge]] = top
            if nsplit > 1 and trial == 4:
                v[[edge - 2, min(edge + 1, K - 1)]] = top - 0.5
                v[edge - 1] = top
            if K >= 3 and trial == 5:                      # three equal maxima, the last one in the last part
                v[[0, K // 2, K - 1]] = top
            out.append((K, nsplit, trial, v))
    return out


@pytest.mark.parametrize("K,nsplit,trial,vals", _cases(), ids=lambda p: None if isinstance(p, np.ndarray) else str(p))
def test_online_top2_and_lse_over_panels_and_parts_equal_the_direct_sort(K, nsplit, trial, vals):
    m, a, m2, a2, lse = _model(vals, nsplit)
    rm, ra, rm2, ra2, rlse = _direct(vals)
    assert (m, a, m2, a2) == (rm, ra, rm2, ra2)
    assert abs(lse - rlse) <= 1e-12 * max(1.0, abs(rlse))


def test_single_label_has_no_runner_up():
    m, a, m2, a2, lse = _model(np.array([0.25]), 1)
    assert (m, a, m2, a2, lse) == (0.25, 0, -np.inf, -1, 0.25)


def _header_arity(name):
    src = open(os.path.join(_ROOT, "include", "lseg_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/lseg_hip.h"
    return len([p for p in m.group(1).split(",") if p.strip()])


@pytest.mark.parametrize("name", ["lseg_forward_labels_conf", "lseg_op_corr_argmax_conf"])
def test_new_entries_are_declared_bound_and_exported_with_matching_arity(name):
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert len(args) == _header_arity(name)
    assert hasattr(_lib.load(), name)
    assert _lib.load().lseg_abi_version() == 1             # additive: the ABI version stays


def test_conf_entries_extend_the_plain_ones_by_three_pointers():
    for plain, conf in (("lseg_forward_labels", "lseg_forward_labels_conf"), ("lseg_op_corr_argmax", "lseg_op_corr_argmax_conf")):
        assert _header_arity(conf) == _header_arity(plain) + 3
