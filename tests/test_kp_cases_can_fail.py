"""CPU, no kernel involved: the bodies of tests/kp_cases.py CAN fail, and the dispatch table they rely on is the source's.

* The restated host rules of kpconv.hip are pinned to the source text; every kernel the file dispatches is reached by a named case.
* A stand-in for ``ml3d.ops`` written in float64 torch passes every body it is given.
* Each deliberately wrong stand-in is rejected by EVERY case that covers its edge, and -- for the float bodies -- by the float
  comparison itself: a finite ``max_abs_delta`` above ``tol``:
    - the walk ends one real column early,
    - kernel point 14 is dropped (the padding slot off by one),
    - a shadow neighbour is support row 0, position and features (what an unconditional clamped load reads),
    - the Gaussian denominator lacks its factor 2,
    - ``max_pool`` skips shadows instead of counting them as zero rows,
    - the adjoint stores its contribution instead of adding it (the last writer wins)."""
import numpy as np
import pytest
import torch

import kp_cases as C
import kp_ref as R


class StandIn:
    """``ml3d.ops``' KPConv entries in float64 (results as float32, like the kernels'); ``wrong``: one of the faults above."""

    def __init__(self, wrong=None):
        self.wrong = wrong

    def _geometry(self, q, s, inds, kp):
        ns = s.shape[0]
        inds = inds.clone()
        if self.wrong == "shadow_is_row0":
            inds[~R.real(inds, ns)] = 0
        if self.wrong == "early_end":
            for row in inds:
                cols = torch.nonzero(R.real(row, ns)).reshape(-1)
                if len(cols):
                    row[cols[-1]] = ns
        return q.double(), s.double(), inds, kp.double()

    def _wf(self, q, s, inds, x, kp, extent, influence, **kw):
        if self.wrong == "gauss_no2":
            kw["gaussian_factor"] = 1.0
        wf = R.weighted(*self._geometry(q, s, inds, kp)[:3], x.double(), kp.double(), extent, influence, **kw)
        if self.wrong == "drop_kp14":
            wf[:, 14] = 0
        return wf

    def kpconv_weighted(self, q, s, inds, x, kp, extent, influence=1):
        return (self._wf(q, s, inds, x, kp, extent, influence).flatten(1) + 0.0).float()      # (+ 0.0: no -0.0, whose bits a row alone need not repeat)

    @staticmethod
    def pack_bf16x3(w):
        return "packed"

    def kpconv_rigid(self, q, s, inds, x, kp, w, bias, extent, act=1, slope=0.1, influence=1, offset_features=None, packed=None):
        kw = {}
        if offset_features is not None:
            off = offset_features.double()
            kw["offsets"] = off[:, :45].reshape(-1, 15, 3) * extent
            kw["modulations"] = 2 * torch.sigmoid(off[:, 45:]) if off.shape[1] > 45 else None
        wf = self._wf(q, s, inds, x, kp, extent, influence, **kw)
        # (the activation in float32, like the kernels' epilogues: an all-shadow row is act(bias) to the bit)
        return R.activation(R.contract(wf, w.double(), None if bias is None else bias.double()).float(), act, slope)

    def kpconv_deformable(self, q, s, inds, x, kp, w, bias, extent, ow, ob, act=1, slope=0.1, influence=1):
        off = self.kpconv_rigid(q, s, inds, x, kp, ow, ob, extent, act=0, influence=influence)
        return self.kpconv_rigid(q, s, inds, x, kp, w, bias, extent, act=act, slope=slope, influence=influence, offset_features=off)

    def kpconv_weighted_backward(self, q, s, inds, dwf, cin, kp, extent, influence=1):
        qd, sd, ii, kd = self._geometry(q, s, inds, kp)
        kw = dict(gaussian_factor=1.0) if self.wrong == "gauss_no2" else {}
        w = R.influences(qd, sd, ii, kd, extent, influence, **kw)
        if self.wrong == "drop_kp14":
            w[:, 14] = 0
        contrib = torch.matmul(w.transpose(1, 2), dwf.double().view(q.shape[0], 15, cin))       # [nq, h, cin]
        ok = R.real(ii, s.shape[0])
        dx = torch.zeros((s.shape[0], cin), dtype=torch.float64)
        if self.wrong == "adjoint_store":
            for qi in range(ii.shape[0]):
                for h in torch.nonzero(ok[qi]).reshape(-1).tolist():
                    dx[int(ii[qi, h])] = contrib[qi, h]
        else:
            dx.index_add_(0, ii[ok].long(), contrib[ok])
        return dx.float()

    def gather_pool(self, x, inds, mode):
        xn, ii = x.numpy(), inds.numpy()
        if mode == "closest":
            return torch.from_numpy(R.closest_pool(xn, ii))
        if self.wrong != "pool_skips_shadows":
            return torch.from_numpy(R.max_pool(xn, ii))
        ok = (ii >= 0) & (ii < xn.shape[0])
        g = np.where(ok[:, :, None], xn[np.where(ok, ii, 0)], -np.inf)
        return torch.from_numpy(g.max(1).astype(np.float32))


# ---- the dispatch table ---------------------------------------------------------------------------------------------------------------
def test_the_restated_host_rules_are_the_text_of_kpconv_hip():
    C.assert_rules_are_the_sources()


def test_every_dispatch_arm_is_reached_by_a_named_case():
    table = C.arms_table()
    missing = [a for a in C.REQUIRED_ARMS if a not in table]
    assert not missing, missing
    for arm in C.REQUIRED_ARMS:
        print("%-32s %s" % (arm, table[arm][0]))
    # what the tables say they are for
    arm = lambda group, i=0: C.arms_of(C.cases_of(group)[i])
    assert all(a.startswith("kp_small_fused") for c in C.cases_of("fused_shape") + C.cases_of("fused_full") for a in C.arms_of(c))
    assert all(C.arms_of(c)[0].startswith("kp_weighted_small") for c in C.cases_of("fused_leaving"))
    assert [C.arms_of(c)[0] for c in C.cases_of("agg_misaligned")] == ["kp_weighted<16,1>", "kp_weighted<32,1>", "kp_weighted<64,1>"]
    assert all(C.arms_of(c)[0].startswith("kp_agg_gemm32") for g in ("b32_full", "b32_tail", "b32_width", "b32_long") for c in C.cases_of(g))
    assert [C.arms_of(c)[0] for c in C.cases_of("b32_leaving")] == ["kp_agg_mfma<2,1> + gemm", "kp_weighted<32,1> + gemm"]
    assert arm("agg_long") == ["kp_agg_mfma<1,1>", "kp_agg_mfma long walk"] and arm("b32_long") == ["kp_agg_gemm32<1>", "kp_agg_gemm32 long walk"]
    assert C.agg_mfma_queries_per_wave(8192)[:2] == (1, 1) and C.agg_mfma_queries_per_wave(8193)[1] == 2
    assert C.agg_gemm32_tiles_per_workgroup(16384)[:2] == (1, 1) and C.agg_gemm32_tiles_per_workgroup(16385)[1] == 2
    assert C.small_fused_lds_bytes(5, 128) == C.SMALL_FUSED_LDS_OPT_IN, "(5, 128): exactly the 48 KiB at which the limit is NOT raised"
    # nq = 9 on the MFMA aggregation: one XCD slice of a single query, three of none
    per = (9 + 7) // 8
    assert [max(0, min(per, 9 - x * per)) for x in range(8)] == [2, 2, 2, 2, 1, 0, 0, 0]


def test_the_row_table_holds_every_kind_at_every_width():
    for h in C.H_WIDTHS:
        g = C.geometry(33, h)
        inds, ns = g["inds"].numpy(), C.NS
        real = (inds >= 0) & (inds < ns)
        assert set(g["kinds"]) == set(C.row_kinds(h))
        last = [int(np.flatnonzero(r)[-1]) if r.any() else -1 for r in real]
        assert real.all(1).any() and (~real).all(1).any() and (h - 1) in last
        assert {c for c in (63, 64, 127, 128) if c < h} <= set(last)
        if h >= 9:
            assert set(inds[~real].tolist()) == set(C.SHADOWS(ns))
            assert any(len(set(r[k].tolist())) < k.sum() for r, k in zip(inds, real)), "duplicates in a row"
            assert any(k.any() and not k[:int(np.flatnonzero(k)[-1]) + 1].all() for k in real), "a shadow before a real column"


# ---- the stand-ins --------------------------------------------------------------------------------------------------------------------
SAMPLE = list(C.CASES)                                # every case of every table, the two long walks included
_ids = lambda cases: ["%s[%s]" % (c["group"], c["id"]) for c in cases]


@pytest.mark.parametrize("group", C.GROUPS)
def test_the_correct_stand_in_passes(group):
    for c in C.cases_of(group):
        C.run_case("cpu", c, StandIn(), report=lambda **kv: None)


def _rejected(case, wrong):
    seen = []
    with pytest.raises(AssertionError):
        C.run_case("cpu", case, StandIn(wrong), report=lambda **kv: seen.append(kv))
    seen = [kv for kv in seen if "tol" in kv]
    assert seen and np.isfinite(seen[0]["max_abs_delta"]) and seen[0]["max_abs_delta"] > seen[0]["tol"], \
        "rejected by the float comparison itself"
    print("%s: max_abs_delta=%.3g tol=%.3g" % (wrong, seen[0]["max_abs_delta"], seen[0]["tol"]))


def _has_rows(c, n=1):
    return c["body"] in C.FLOAT_BODIES and c["kw"]["h"] >= 1 and c["kw"].get("nq", 33) >= n


EARLY = [c for c in SAMPLE if _has_rows(c)]
SHADOWED = [c for c in SAMPLE if _has_rows(c, 3)]                       # (rows 1 and 2 of a case hold shadows)
GAUSSIAN = [c for c in SAMPLE if _has_rows(c) and c["kw"].get("influence") == 2]
ADJOINT = [c for c in SAMPLE if c["body"] == "adjoint"]
POOLS = [c for c in C.CASES if c["body"] == "pool"]


@pytest.mark.parametrize("case", EARLY, ids=_ids(EARLY))
def test_a_walk_that_ends_one_real_column_early_is_rejected(case):
    _rejected(case, "early_end")


@pytest.mark.parametrize("case", EARLY, ids=_ids(EARLY))
def test_a_dropped_kernel_point_14_is_rejected(case):
    _rejected(case, "drop_kp14")


@pytest.mark.parametrize("case", SHADOWED, ids=_ids(SHADOWED))
def test_a_shadow_read_as_support_row_0_is_rejected(case):
    _rejected(case, "shadow_is_row0")


@pytest.mark.parametrize("case", GAUSSIAN, ids=_ids(GAUSSIAN))
def test_a_gaussian_denominator_without_its_factor_2_is_rejected(case):
    _rejected(case, "gauss_no2")


@pytest.mark.parametrize("case", ADJOINT, ids=_ids(ADJOINT))
def test_an_adjoint_that_stores_instead_of_adding_is_rejected(case):
    _rejected(case, "adjoint_store")


@pytest.mark.parametrize("case", POOLS, ids=_ids(POOLS))
def test_a_max_pool_that_skips_shadows_is_rejected(case):
    with pytest.raises(AssertionError, match="pool"):
        C.run_case("cpu", case, StandIn("pool_skips_shadows"))
