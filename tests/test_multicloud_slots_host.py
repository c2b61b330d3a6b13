"""CPU: the slot table and the argument checks that ``RandLANet.inference_many`` and ``KPFCNN.inference_many`` share
(ml3d/torch/models/_multicloud.py), driven on CPU tensors with fake clouds -- no GPU, no emulator.  The multi-cloud GPU runs rarely
admit a cloud into a freed slot while another survives; here that is the whole test: clouds of 5, 7, 3 and 4 rows, two slots."""
import types

import numpy as np
import pytest
import torch

from ml3d.torch.models._multicloud import CloudSlots, check_many_args

ROWS = (5, 7, 3, 4)
CLASSES = 3
ARRAYS = ("points", "possibility", "label", "votes")


def _clouds(with_feat):
    g = torch.Generator().manual_seed(7)
    out = []
    for i, n in enumerate(ROWS):
        out.append(dict(cloud=i, n=n, proj_inds=np.random.default_rng(i).integers(0, n, size=2 * n + 1),
                        points=torch.rand((n, 3), generator=g), possibility=torch.rand(n, generator=g, dtype=torch.float64),
                        label=torch.randint(0, CLASSES, (n,), generator=g),
                        feat=torch.rand((n, 2), generator=g) if with_feat else None))
    return out


def _table(with_feat):
    clouds = _clouds(with_feat)
    own = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in c.items()} for c in clouds]     # what each cloud brought
    waiting, gone = iter(clouds), []
    t = CloudSlots(2, lambda: next(waiting, None), lambda st, result, poss: gone.append((st, result, poss)), torch.device("cpu"), CLASSES)
    return t, own, gone


def _fill_votes(t, seed):
    """Distinct votes in every row, as the vote updates of some rounds would leave them."""
    g = torch.Generator().manual_seed(seed)
    t.buf["votes"].copy_(torch.rand(t.buf["votes"].shape, generator=g).to(torch.float16))


def _names(with_feat):
    return ARRAYS + (("feat",) if with_feat else ())


def _rows_of(t, slot, names):
    a, b = t.rows(slot)
    return {name: t.buf[name][a:b].clone() for name in names}


@pytest.mark.parametrize("with_feat", [False, True], ids=["feat=None", "feat"])
def test_a_freed_slot_is_refilled_and_the_survivor_moves_bit_for_bit(with_feat):
    names = _names(with_feat)
    t, own, gone = _table(with_feat)
    # the initial fill: clouds 0 and 1, back to back
    assert [st["cloud"] for st in t.slots] == [0, 1] and t.active() == [0, 1]
    assert t.splits.dtype == np.int64 and t.splits.tolist() == [0, 5, 12] and t.rows(1) == (5, 12)
    for name in names:
        if name != "votes":
            assert torch.equal(t.buf[name], torch.cat([own[0][name], own[1][name]]))
        assert all(name not in st for st in t.slots)                  # the table holds the arrays, not the states
    assert t.buf["votes"].dtype == torch.float16 and tuple(t.buf["votes"].shape) == (12, CLASSES) and not t.buf["votes"].any()
    if not with_feat:
        assert t.buf["feat"] is None
    _fill_votes(t, 1)
    t.buf["possibility"].add_(1.0)                                    # (the loop bumps them in place)
    cloud0, cloud1 = _rows_of(t, 0, names), _rows_of(t, 1, names)

    # slot 0 finishes, cloud 2 takes it: one rebuild, the survivor's rows at their new offsets
    assert t.replace_finished([0]) is True
    assert [st["cloud"] for st in t.slots] == [2, 1] and t.splits.tolist() == [0, 3, 10] and t.rows(1) == (3, 10)
    moved, fresh = _rows_of(t, 1, names), _rows_of(t, 0, names)
    for name in names:
        assert moved[name].dtype == cloud1[name].dtype and torch.equal(moved[name], cloud1[name]), name
        assert t.buf[name].is_contiguous() and t.buf[name].shape[0] == 10
        if name != "votes":
            assert torch.equal(fresh[name], own[2][name]), name
    assert not fresh["votes"].any()
    # the retired cloud's result: ITS votes through ITS proj_inds, its possibilities as they stood
    (st, result, poss), = gone
    probs = cloud0["votes"].numpy()
    assert st["cloud"] == 0 and poss.dtype == np.float64 and np.array_equal(poss, cloud0["possibility"].numpy())
    assert result["predict_scores"].dtype == np.float16 and np.array_equal(result["predict_scores"], probs[own[0]["proj_inds"]])
    assert np.array_equal(result["predict_labels"], np.argmax(probs, 1)[own[0]["proj_inds"]])
    assert sorted(result) == ["predict_labels", "predict_scores"]

    # slot 1 finishes, cloud 3 takes it
    _fill_votes(t, 2)
    cloud2, cloud1 = _rows_of(t, 0, names), _rows_of(t, 1, names)
    assert t.replace_finished([1]) is True
    assert [st["cloud"] for st in t.slots] == [2, 3] and t.splits.tolist() == [0, 3, 7]
    kept = _rows_of(t, 0, names)
    for name in names:
        assert torch.equal(kept[name], cloud2[name]), name
    assert gone[1][0]["cloud"] == 1 and np.array_equal(gone[1][1]["predict_scores"], cloud1["votes"].numpy()[own[1]["proj_inds"]])

    # slot 0 finishes with no cloud left: nothing is rebuilt, the slot only leaves the active list
    _fill_votes(t, 3)
    buf, splits, cloud3 = t.buf, t.splits, _rows_of(t, 1, names)
    assert t.replace_finished([0]) is False
    assert t.buf is buf and t.splits is splits and t.slots[0] is None and t.active() == [1]
    assert all(t.buf[name].shape[0] == 7 for name in names)
    assert gone[2][0]["cloud"] == 2
    # ... and in the next set of arrays it has no rows
    t.rebuild()
    assert t.splits.tolist() == [0, 0, 4] and t.rows(0) == (0, 0) and t.rows(1) == (0, 4)
    for name in names:
        assert torch.equal(t.buf[name], cloud3[name]), name
    assert t.replace_finished([1]) is False and t.active() == [] and [g[0]["cloud"] for g in gone] == [0, 1, 2, 3]
    assert np.array_equal(gone[3][1]["predict_scores"], cloud3["votes"].numpy()[own[3]["proj_inds"]])


def test_check_many_args_messages():
    model = types.SimpleNamespace(device=torch.device("cuda"), training=False)
    draws = []

    def draw(n):
        draws.append(n)
        return list(range(n))

    assert check_many_args("X.inference_many", model, 3, 2.0, None, draw) == (2, [0, 1, 2]) and draws == [3]
    assert check_many_args("X.inference_many", model, 2, 256, [5, 6], draw) == (256, [5, 6]) and draws == [3]
    with pytest.raises(RuntimeError, match=r"^X\.inference_many needs an MI355X device"):
        check_many_args("X.inference_many", types.SimpleNamespace(device=torch.device("cpu"), training=False), 1, 1, None, draw)
    with pytest.raises(RuntimeError, match=r"^X\.inference_many: call model\.eval\(\) first$"):
        check_many_args("X.inference_many", types.SimpleNamespace(device=torch.device("cuda"), training=True), 1, 1, None, draw)
    for bad in (0, 257):
        with pytest.raises(ValueError, match=r"^X\.inference_many: 1 <= max_in_flight <= 256$"):
            check_many_args("X.inference_many", model, 1, bad, None, draw)
    with pytest.raises(ValueError, match=r"^X\.inference_many: one seed per cloud$"):
        check_many_args("X.inference_many", model, 2, 1, [1], draw)
    assert draws == [3]
