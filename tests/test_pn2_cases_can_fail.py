"""CPU, no kernel involved: the ball-query and set-abstraction bodies of tests/pn2_cases.py CAN fail.  Each body runs against a
stand-in written in numpy / float64 torch: the CORRECT stand-in passes (so the body judges what it is given, nothing else), and
each deliberately wrong one is rejected --

* ``d2 <= r * r`` instead of ``d2 < r * r``       (the point at exactly the radius becomes a hit),
* the hits of a ball in ascending DISTANCE instead of ascending index,
* the maximum over nsample - 1 neighbours instead of nsample."""
import numpy as np
import pytest
import torch

import pn2_cases as C
import pn2_ref


class BallStandIn:
    def __init__(self, **wrong):
        self.wrong = wrong

    def ball_query(self, xyz, new_xyz, radius, nsample):
        many = isinstance(radius, (list, tuple))
        outs = [torch.from_numpy(pn2_ref.ball_query(xyz.numpy(), new_xyz.numpy(), r, k, **self.wrong))
                for r, k in zip(radius if many else [radius], nsample if many else [nsample])]
        return outs if many else outs[0]


class SaStandIn:
    """``pack_sa_weights`` / ``pn2_sa_mlp_max`` of ``ml3d.ops`` in float64: Wx (p - c) + y, two more layers, the maximum."""

    def __init__(self, drop_last=0):
        self.drop_last = drop_last

    @staticmethod
    def pack_sa_weights(w_x, b1, w2, b2, w3, b3, nsample):
        return dict(w_x=w_x, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3)

    def pn2_sa_mlp_max(self, y, xyz, centres, idx, params, out=None):
        p = {k: v.double() for k, v in params.items()}
        b, m, ns = idx.shape
        n = xyz.shape[1]
        rows = (idx.long() + torch.arange(b)[:, None, None] * n).reshape(-1)
        h = (xyz.double().reshape(b * n, 3).index_select(0, rows).view(b, m, ns, 3) - centres.double()[:, :, None, :]) @ p["w_x"]
        if y is not None:
            h = h + y.double().index_select(0, rows).view(b, m, ns, -1)
        h = torch.relu(h + p["b1"])
        h = torch.relu(h @ p["w2"] + p["b2"])
        h = torch.relu(h @ p["w3"] + p["b3"])
        res = h[:, :, :ns - self.drop_last].max(2)[0].reshape(b * m, -1).float()
        if out is None:
            return res
        out.copy_(res)
        return out


def _ball_bodies(impl):
    C.check_ball_query("cpu", 1000, 67, impl)
    C.check_ball_query_properties("cpu", impl)
    C.check_ball_query_boundary_and_duplicates("cpu", impl)
    C.check_ball_query_batch("cpu", impl)


def test_the_correct_stand_ins_pass():
    _ball_bodies(BallStandIn())
    C.check_sa("cpu", 3, (32, 32, 64), 16, 67, SaStandIn())
    C.check_sa("cpu", 96, (64, 96, 128), 32, 5, SaStandIn())


def test_less_or_equal_instead_of_less_is_rejected():
    with pytest.raises(AssertionError, match="boundary"):
        C.check_ball_query_boundary_and_duplicates("cpu", BallStandIn(strict=False))


@pytest.mark.parametrize("body", [lambda i: C.check_ball_query("cpu", 1000, 67, i), lambda i: C.check_ball_query("cpu", 130, 8, i),
                                  lambda i: C.check_ball_query_properties("cpu", i), lambda i: C.check_ball_query_batch("cpu", i)],
                         ids=["n1000", "n130", "properties", "batch"])
def test_hits_in_distance_order_are_rejected(body):
    with pytest.raises(AssertionError):
        body(BallStandIn(by_distance=True))


@pytest.mark.parametrize("ns", C.SA_NSAMPLE)
@pytest.mark.parametrize("cf,widths", C.SA_CASES[:3], ids=["-".join(map(str, w)) for _, w in C.SA_CASES[:3]])
def test_a_maximum_over_one_neighbour_less_is_rejected(cf, widths, ns):
    seen = []
    with pytest.raises(AssertionError):
        C.check_sa("cpu", cf, widths, ns, 67, SaStandIn(drop_last=1), report=lambda **kv: seen.append(kv))
    assert seen and seen[0]["max_abs_delta"] > seen[0]["tol"], "rejected by the float comparison itself"
    assert np.isfinite(seen[0]["max_abs_delta"])
