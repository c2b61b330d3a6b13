"""CPU, no library: the bodies of tests/finish_cases.py run against numpy stand-ins for ``ops.vote_project``.  The right one passes
every case; each wrong one is rejected by every case that covers its edge and by no other (so a case fails FOR that edge):

* the LAST maximum instead of the first        * labels taken without the projection
* NaN ignored                                  * scores through float32 and back, NaN canonicalised
* -0 < +0                                      * a row base rounded down to 4 bytes
"""
import numpy as np
import pytest
import torch

import finish_cases as F

DATA_CASES = ("sizes", "base_offsets", "values", "projections", "labels_only")


def _rows(votes, round_base_down=False):
    """The votes as uint16 bits [n_sub, C], read row by row from the tensor's storage at the half-word offset a kernel would use."""
    n_sub, C = votes.shape
    flat = torch.as_strided(votes, (votes.untyped_storage().nbytes() // 2,), (1,), 0).numpy().view(np.uint16)
    out = np.empty((n_sub, C), np.uint16)
    for r in range(n_sub):
        off = votes.storage_offset() + r * C
        if round_base_down:
            off &= ~1
        out[r] = flat[off:off + C]
    return out


def _first_max(v):
    return np.argmax(v, 1)


def _last_max(v):
    return v.shape[1] - 1 - np.argmax(v[:, ::-1], 1)


def _nan_ignored(v):
    return np.argmax(np.where(np.isnan(v), -np.inf, v.astype(np.float32)), 1)


def _neg_zero_less(v):
    f = v.astype(np.float64)
    f[v.view(np.uint16) == F.H_NEG_ZERO] = -1e-30
    return np.argmax(f, 1)


def _via_float32(rows):
    f = rows.astype(np.float32)
    f[np.isnan(f)] = np.nan                   # the canonical quiet NaN
    return f.astype(np.float16)


def standin(argmax=_first_max, project_labels=True, scores_of=lambda rows: rows, round_base_down=False):
    def op(votes, proj, out_labels=None, out_scores=None, scores=True):
        v = _rows(votes, round_base_down).view(np.float16)
        p = proj.numpy()
        lab = argmax(v)
        lab = lab[p] if project_labels else lab[np.minimum(np.arange(p.size), len(v) - 1)]
        if out_labels is None:
            out_labels = torch.empty(p.size, dtype=torch.uint8)
        out_labels.copy_(torch.from_numpy(lab.astype(np.uint8)))
        if not scores:
            return out_labels, None
        if out_scores is None:
            out_scores = torch.empty((p.size, v.shape[1]), dtype=torch.float16)
        out_scores.copy_(torch.from_numpy(np.ascontiguousarray(scores_of(v[p]))))
        return out_labels, out_scores
    return op


WRONG = {
    "last maximum": (standin(argmax=_last_max), DATA_CASES),                       # every case has all-zero rows and C > 1
    "NaN ignored": (standin(argmax=_nan_ignored), ("values",)),
    "-0 < +0": (standin(argmax=_neg_zero_less), ("values",)),
    "no projection": (standin(project_labels=False), DATA_CASES),
    "scores via float32": (standin(scores_of=_via_float32), ("values",)),
    "row base rounded down": (standin(round_base_down=True), DATA_CASES),          # every case has rows at odd half-word offsets
}


@pytest.mark.parametrize("case", DATA_CASES)
def test_the_right_standin_passes(case):
    F.CASES[case]("cpu", standin())


@pytest.mark.parametrize("case", DATA_CASES)
@pytest.mark.parametrize("name", sorted(WRONG))
def test_a_wrong_standin_is_rejected_where_its_edge_is_covered(name, case):
    op, covered = WRONG[name]
    if case in covered:
        with pytest.raises(AssertionError):
            F.CASES[case]("cpu", op)
    else:
        F.CASES[case]("cpu", op)
