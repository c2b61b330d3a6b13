"""CPU, no kernel involved: the bodies of tests/train_cases.py CAN fail, and the dispatch table they rely on is the source's.

* The restated host rules of train.hip (and of the four randla.hip entries) are pinned to the source text; every ``__global__`` of
  train.hip is in ``REQUIRED_ARMS`` and every required arm is reached by a named case.
* The written-out gradients of tests/train_ref.py equal torch's autograd in float64 where autograd's rule is defined (no ties).
* A stand-in for ``train_cases.Product`` written in float64 passes every body it is given.
* Each deliberately wrong stand-in is rejected by EVERY case that covers its edge, by the float comparison itself -- a finite
  ``max_abs_delta`` above ``tol``:
    - a scatter stores instead of adding (the last writer wins),
    - a shadow index is row 0 (what an unconditional clamped access touches),
    - the max adjoint sends the gradient to the LAST maximal neighbour,
    - the max adjoint gives a winning shadow's gradient to a real row with the same value,
    - the LeakyReLU mask is taken from the BatchNorm input instead of its output,
    - the BatchNorm backward omits xhat mean(g' xhat),
    - the variance is the unbiased one,
    - ``gemm_tn`` drops the last row of an odd m,
    - the attention backward omits ``- out`` in gs,
    - the attention's partial sum skips the last workgroup's private partial,
    - the deformed kernel-point gradient ignores the clamp's mask."""
import numpy as np
import pytest
import torch

import train_cases as C
import train_ref as R

F64 = torch.float64


class StandIn:
    """``train_cases.Product`` in float64 (results as float32, like the kernels'); ``wrong``: one of the faults above."""

    def __init__(self, wrong=None):
        self.wrong = wrong

    def _is(self, what):
        return self.wrong == what

    def gemm_tn(self, a, b, k, n, ldc, col_sums):
        a, b = a[:, :k], b[:, :n]
        m = a.shape[0]
        keep = m - 1 if self._is("gemm_odd_row") and m % 2 else m
        c = torch.full((k, ldc), C.SENTINEL, dtype=torch.float32)
        c[:, :n] = R.gemm_tn(a[:keep], b[:keep], F64)[0].float()
        return c, R.gemm_tn(a, b, F64)[1].float() if col_sums else None

    def bn_forward(self, x, gamma, beta, eps, slope):
        y, _, mean, var, invstd = R.bn_forward(x, gamma, beta, eps, slope, F64, unbiased=self._is("bn_unbiased"))
        return y.float(), mean.float(), var.float(), invstd.float()

    def bn_backward(self, x, y, gy, gamma, beta, mean, invstd, eps, slope):
        gx, gg, gb = R.bn_backward(x, gy, gamma, beta, eps, slope, F64, mask_from_input=self._is("bn_mask_input"),
                                   drop_xhat_term=self._is("bn_no_xhat"))
        return gx.float(), None if gamma is None else gg.float(), None if beta is None else gb.float()

    def bn_function(self, x, gamma, beta, rm, rv, momentum, eps, slope, gy):
        y, mean, var, _ = self.bn_forward(x, gamma, beta, eps, slope)
        gx, gg, gb = self.bn_backward(x, y, gy, gamma, beta, None, None, eps, slope)
        rm2, rv2 = R.running_update(rm, rv, mean, var, x.shape[0], momentum, F64)
        return y, gx, gg, gb, rm2.float(), rv2.float()

    @staticmethod
    def _index(idx, stride, m):
        return idx.reshape(-1)[::stride][:m] if m else idx.reshape(-1)[:0]

    def gather_rows(self, x, idx, stride, m):
        return R.gather_rows(x, self._index(idx, stride, m))

    def scatter_add_rows(self, g, n_src, idx, stride, m):
        return R.scatter_add_rows(g, n_src, self._index(idx, stride, m), F64, store=self._is("scatter_store"),
                                  shadow_is_row0=self._is("shadow_row0")).float()

    def pool_forward(self, x, inds, mode):
        return R.max_pool(x, inds) if mode == "max" else R.gather_rows(x, inds[:, 0])

    def pool_backward(self, x, inds, mode, g):
        if mode == "max":
            return R.max_pool_adjoint(x, inds, g, F64, last=self._is("max_last"), shadow_to_real=self._is("max_shadow_to_real"),
                                      store=self._is("scatter_store")).float()
        if inds.shape[1] == 0:
            return torch.zeros(x.shape)
        return self.scatter_add_rows(g, x.shape[0], inds, inds.shape[1], inds.shape[0])

    def attention_forward(self, f, enc, idx, w, bias):
        return R.attention_forward(f, enc, idx, w, bias, F64, shadow_is_row0=self._is("shadow_row0"))[0].float()

    def attention_backward(self, f, enc, idx, w, bias, out, g):
        kw = dict(no_minus_out=self._is("attn_no_minus_out"), shadow_is_row0=self._is("shadow_row0"))
        gf, genc, gw, gb = R.attention_backward(f, enc, idx, w, bias, g, F64, **kw)
        if self._is("attn_skip_last_group"):
            B, n, c1 = f.shape
            d = c1 + enc.shape[3]
            _, _, tiles, groups, _ = C.attn_plan(B * n, d)
            per = 4 if d <= 16 else 2
            last = torch.zeros(B * n, dtype=torch.bool)
            for t in range(groups - 1, tiles, groups):
                last[t * per:(t + 1) * per] = True
            gw = gw - R.attention_backward(f, enc, idx, w, bias, g * last.view(B, n, 1).float(), F64)[2]
        return gf.float(), genc.float(), gw.float(), None if bias is None else gb.float()

    def deformed(self, x, dkp, q, s, inds, extent, dwf):
        nq, h = inds.shape
        _, dist, _, ok = R.deformed_geometry(q, s, inds, dkp, extent, F64) if nq and h else (0, torch.ones(1), 0, torch.zeros(1, dtype=torch.bool))
        without = [(qi, hi, ki) for qi, ki, hi in torch.nonzero((dist == 0) & ok).tolist()]       # (a term at dist == 0 contributes nothing)
        dx, gkp = R.deformed_backward(q, s, inds, x, dkp, extent, dwf, F64, without=without, ignore_clamp=self._is("deform_no_clamp"))
        wf = R.deformed_forward(q, s, inds, x, dkp, extent, F64)
        return wf.flatten(1).float(), dx.float(), gkp.float()

    def regulariser(self, dkp, q, s, inds, extent, repulse):
        r = R.regulariser(q, s, inds, dkp, extent, repulse, F64)
        return {key: r[key].float() for key in ("fit", "rep", "min_d2", "gfit", "grep")}

    def gather_max(self, feat, idx, n_out, g):
        return R.gather_max(feat, idx, n_out), R.gather_max_adjoint(feat, idx, n_out, g, F64, last=self._is("max_last")).float()

    def attentive_pool(self, scores, x, g):
        gs, gx = R.attentive_pool_backward(scores, x, g, F64)
        return R.attentive_pool(scores, x, F64)[0].float(), gs.float(), gx.float()


# ---- the dispatch table ---------------------------------------------------------------------------------------------------------------
def test_the_restated_host_rules_are_the_text_of_the_sources():
    C.assert_rules_are_the_sources()


def test_every_kernel_and_every_named_property_is_reached_by_a_case():
    table = C.arms_table()
    missing = [a for a in C.REQUIRED_ARMS if a not in table]
    assert not missing, missing
    for arm in C.REQUIRED_ARMS:
        print("%-48s %s" % (arm, table[arm][0]))
    kernels = C.train_globals()
    assert len(kernels) == 14 and len(set(kernels)) == 14, kernels
    for name in kernels:
        assert any(a == name or a.startswith(name + "<") for a in C.REQUIRED_ARMS), name
    # what the tables say they are for
    only = lambda group: C.cases_of(group)[0]["kw"]
    assert C.gemm_plan(**only("gemm_by_tiles"))[3] == "tiles" and C.gemm_plan(1000, 130, 97)[3] == "rows"
    assert C.gemm_plan(129, 64, 64)[:2] == (2, 66) and C.gemm_plan(3, 33, 65)[:2] == (1, 4), "rows per slice are rounded to even"
    assert C.tr_blocks(C.BN_CAP["rows"] * C.BN_CAP["c"], 1024, 4096) == 4096 and C.BN_CAP["rows"] * C.BN_CAP["c"] > 4096 * 1024
    assert C.GATHER_CAP["nq"] * C.GATHER_CAP["c"] > 8192 * 256
    assert C.attn_plan(2050, 18)[2:] == (1025, 1025, 3) and C.attn_plan(1282, 256)[2:] == (641, 640, 2) and C.attn_plan(8198, 6)[2:4] == (2050, 2048)
    assert [C.attn_plan(bn, 96)[4] for bn in (64, 65)] == [1, 2] and C.attn_plan(64, 96)[3] == 32
    classes = {C.attn_plan(34, c1 + c2)[:2] for c1, c2 in C.ATTN_SHAPES}
    assert classes == {(64, 16), (64, 64), (64, 128), (32, 256)}
    assert max(c1 for c1, c2 in C.ATTN_SHAPES if c1 + c2 > 128) == C.AS_C1MAX
    assert C.reduce_blocks(2, 512) == 1 and C.reduce_blocks(3, 1024) == 1 and C.reduce_blocks(1000, 340) == 42 and C.reduce_blocks(7, 5) == 1


def test_the_written_out_gradients_are_autograd_s_in_float64():
    rng = np.random.default_rng(0)
    T = lambda *shape: torch.from_numpy(rng.standard_normal(shape))
    # BatchNorm + LeakyReLU
    x, gam, bet, gy = T(9, 5).requires_grad_(True), T(5).requires_grad_(True), T(5).requires_grad_(True), T(9, 5)
    y = torch.nn.functional.leaky_relu(torch.nn.functional.batch_norm(x, None, None, gam, bet, True, 0.1, 1e-5), 0.2)
    want = torch.autograd.grad(y, (x, gam, bet), gy)
    assert torch.allclose(y, R.bn_forward(x.detach(), gam.detach(), bet.detach(), 1e-5, 0.2, F64)[0], atol=1e-12)
    for a, b in zip(R.bn_backward(x.detach(), gy, gam.detach(), bet.detach(), 1e-5, 0.2, F64), want):
        assert torch.allclose(a, b, atol=1e-11)
    # the attention stage, shadows included (a padded zero row)
    B, n, c1, c2 = 2, 7, 3, 5
    f, enc, w, bias, g = T(B, n, c1).requires_grad_(True), T(B, n, 16, c2).requires_grad_(True), T(8, 8).requires_grad_(True), T(8).requires_grad_(True), T(B, n, 8)
    idx = C._i32(C._shadowed(rng, rng.integers(0, n, (B, n, 16)), n))
    pad = torch.cat([f, torch.zeros(B, 1, c1, dtype=F64)], 1)
    xx = torch.cat([pad[torch.arange(B)[:, None, None], torch.where(R.real(idx, n), idx, torch.full_like(idx, n)).long()], enc], -1)
    out = (torch.softmax(xx @ w.t() + bias, 2) * xx).sum(2)
    want = torch.autograd.grad(out, (f, enc, w, bias), g)
    d = lambda t: t.detach()
    assert torch.allclose(out, R.attention_forward(d(f), d(enc), idx, d(w), d(bias), F64)[0], atol=1e-12)
    for a, b in zip(R.attention_backward(d(f), d(enc), idx, d(w), d(bias), g, F64), want):
        assert torch.allclose(a, b, atol=1e-11)
    # the deformed aggregation (no support on a kernel point, nothing at the clamp)
    _, q, s, inds, dkp, x, dwf, _ = C.deform_inputs(5, 9, 7)
    xd, kd = x.double().requires_grad_(True), dkp.double().requires_grad_(True)
    ok = R.real(inds, s.shape[0])
    nb = s.double()[torch.where(ok, inds, torch.zeros_like(inds)).long()] - q.double()[:, None]
    wgt = torch.clamp(1 - torch.sqrt(((nb[:, None] - kd[:, :, None]) ** 2).sum(3)) / C.EXTENT, min=0) * ok[:, None].double()
    wf = wgt @ xd[torch.where(ok, inds, torch.zeros_like(inds)).long()]
    want = torch.autograd.grad(wf, (xd, kd), dwf.double())
    assert torch.allclose(wf, R.deformed_forward(q, s, inds, x, dkp, C.EXTENT, F64), atol=1e-12)
    for a, b in zip(R.deformed_backward(q, s, inds, x, dkp, C.EXTENT, dwf, F64), want):
        assert torch.allclose(a, b, atol=1e-10)
    # the regulariser (clear minima)
    q, s, inds, dkp, _ = C.reg_inputs(6, 5, 14, True)
    kd = dkp.double().requires_grad_(True)
    far = torch.cat([s.double(), torch.full((1, 3), 1e6, dtype=F64)])
    nb = far[torch.where(R.real(inds, len(s)), inds, torch.full_like(inds, len(s))).long()] - q.double()[:, None]
    min_d2 = ((nb[:, :, None] - kd[:, None]) ** 2).sum(3).min(1)[0]
    locs, rep = kd / C.REG_EXTENT, 0
    for i in range(6):
        others = torch.cat([locs[:, :i], locs[:, i + 1:]], 1).detach()
        rep = rep + (torch.clamp_max(torch.sqrt(((others - locs[:, i:i + 1]) ** 2).sum(2)) - C.REG_REPULSE, 0.0) ** 2).sum()
    r = R.regulariser(q, s, inds, dkp, C.REG_EXTENT, C.REG_REPULSE, F64)
    assert torch.allclose(r["min_d2"], min_d2) and torch.allclose(r["rep"] * 30, rep)
    rows = torch.tensor([True, True, False, True, True])              # (row 2 is all shadows: every neighbour ties, autograd's rule is its own)
    assert torch.allclose(r["gfit"][rows], torch.autograd.grad(min_d2.sum() / C.REG_EXTENT ** 2, kd, retain_graph=True)[0][rows], atol=1e-10)
    assert torch.allclose(r["grep"], torch.autograd.grad(rep, kd)[0], atol=1e-10)
    # attentive pooling
    sc, xx, g = T(4, 6, 3).requires_grad_(True), T(4, 6, 3).requires_grad_(True), T(4, 3)
    want = torch.autograd.grad((torch.softmax(sc, 1) * xx).sum(1), (sc, xx), g)
    for a, b in zip(R.attentive_pool_backward(d(sc), d(xx), g, F64), want):
        assert torch.allclose(a, b, atol=1e-12)


# ---- the stand-ins --------------------------------------------------------------------------------------------------------------------
_ids = lambda cases: ["%s[%s]" % (c["group"], c["id"]) for c in cases]


@pytest.mark.parametrize("group", C.GROUPS)
def test_the_correct_stand_in_passes(group):
    for c in C.cases_of(group):
        seen = []
        C.run_case("cpu", c, StandIn(), report=lambda **kv: seen.append(kv))
        assert len(seen) == C.comparisons(c), (c["id"], len(seen))


def _rejected(case, wrong):
    seen = []
    with pytest.raises(AssertionError):
        C.run_case("cpu", case, StandIn(wrong), report=lambda **kv: seen.append(kv))
    assert seen and "tol" in seen[-1] and np.isfinite(seen[-1]["max_abs_delta"]) and seen[-1]["max_abs_delta"] > seen[-1]["tol"], \
        "rejected by the float comparison itself"
    print("%s: %s max_abs_delta=%.3g tol=%.3g" % (wrong, seen[-1]["name"], seen[-1]["max_abs_delta"], seen[-1]["tol"]))


_of = lambda *bodies: [c for c in C.CASES if c["body"] in bodies]
_kw = lambda c, key, default: c["kw"].get(key, default)
COLLIDING = [c for c in _of("gathers") if _kw(c, "nq", C.GATHER_NQ) > 8 and _kw(c, "n", 1) and c["kw"]["h"]]      # rows 5 and 6 list the same
SHADOWED = [c for c in COLLIDING if c["group"] != "gathers_cap"] + _of("attention")
TIES = [c for c in COLLIDING if c["kw"]["h"] >= 3] + [c for c in _of("gather_max") if c["kw"]["n_out"]]
SHADOW_WINS = [c for c in COLLIDING if c["kw"]["h"] >= 3]
BN_ACT = [c for c in _of("bn", "bn_function") if c["kw"]["slope"] is not None]
BN_ALL = _of("bn", "bn_function")
ODD_M = [c for c in _of("gemm") if c["kw"]["m"] % 2]
ATTENTION = _of("attention")
DEFORMED = [c for c in _of("deformed") if c["kw"]["nq"] and c["kw"]["h"]]


@pytest.mark.parametrize("case", COLLIDING, ids=_ids(COLLIDING))
def test_a_scatter_that_stores_instead_of_adding_is_rejected(case):
    _rejected(case, "scatter_store")


@pytest.mark.parametrize("case", SHADOWED, ids=_ids(SHADOWED))
def test_a_shadow_index_read_as_row_0_is_rejected(case):
    _rejected(case, "shadow_row0")


@pytest.mark.parametrize("case", TIES, ids=_ids(TIES))
def test_a_max_adjoint_that_picks_the_last_maximal_neighbour_is_rejected(case):
    _rejected(case, "max_last")


@pytest.mark.parametrize("case", SHADOW_WINS, ids=_ids(SHADOW_WINS))
def test_a_max_adjoint_that_hands_a_winning_shadow_s_gradient_to_a_real_row_is_rejected(case):
    _rejected(case, "max_shadow_to_real")


@pytest.mark.parametrize("case", BN_ACT, ids=_ids(BN_ACT))
def test_a_leaky_relu_mask_taken_from_the_batchnorm_input_is_rejected(case):
    _rejected(case, "bn_mask_input")


@pytest.mark.parametrize("case", BN_ALL, ids=_ids(BN_ALL))
def test_a_batchnorm_backward_without_the_xhat_term_is_rejected(case):
    _rejected(case, "bn_no_xhat")


@pytest.mark.parametrize("case", BN_ALL, ids=_ids(BN_ALL))
def test_an_unbiased_variance_is_rejected(case):
    _rejected(case, "bn_unbiased")


@pytest.mark.parametrize("case", ODD_M, ids=_ids(ODD_M))
def test_a_gemm_tn_that_drops_the_last_row_of_an_odd_m_is_rejected(case):
    _rejected(case, "gemm_odd_row")


@pytest.mark.parametrize("case", ATTENTION, ids=_ids(ATTENTION))
def test_an_attention_backward_without_minus_out_is_rejected(case):
    _rejected(case, "attn_no_minus_out")


@pytest.mark.parametrize("case", ATTENTION, ids=_ids(ATTENTION))
def test_a_partial_sum_that_skips_the_last_group_is_rejected(case):
    _rejected(case, "attn_skip_last_group")


@pytest.mark.parametrize("case", DEFORMED, ids=_ids(DEFORMED))
def test_a_kernel_point_gradient_that_ignores_the_clamp_is_rejected(case):
    _rejected(case, "deform_no_clamp")
