"""CPU: ops._settle_dict_share - one layer's share of a shared dictionary's gradient against the dictionary's cell - over every
combination of its inputs.  Outside a backward pass the pass id is -1 on the writing and the reading side, so the cell works
on plain CPU tensors; the multi-layer launch is stubbed."""
import itertools

import pytest
import torch

SHARE, MULTI, BUF = 1.0, 10.0, 100.0        # distinct powers of ten: a sum shows every addend and how often it was added


def _t(v):
    return torch.full((2, 3), v)


# (parked and includes_cell together is no state: a parked share has no tensor a launch could have added the buffer into)
@pytest.mark.parametrize("first,parked,includes_cell,has_buf,has_items",
                         [c for c in itertools.product((True, False), repeat=5) if not (c[1] and c[2])])
def test_settle_dict_share(first, parked, includes_cell, has_buf, has_items, monkeypatch):
    from kp_gnn_amd import ops
    calls = []

    def multi(items, n_dict):
        calls.append((list(items), n_dict))
        return _t(MULTI)

    monkeypatch.setattr(ops, "dict_grad_multi_raw", multi)
    cell = ops._SlotGradCell()
    buf = _t(BUF) if has_buf else None
    cell.buf = buf
    n_items = (2 if has_items else 0) + (1 if parked else 0)          # other layers' parked shares, and this layer's own
    for i in range(n_items):
        cell.park_dict(("uid", i), ("theta", i), ("gh", i))
    # (a launch that was given the cell's buffer wrote its result INTO it: the share IS the buffer, holding both)
    grad = None if parked else (buf.add_(SHARE) if (includes_cell and has_buf) else _t(SHARE))
    share = ops._DictShare(grad, includes_cell=includes_cell, parked=parked)

    got = ops._settle_dict_share(cell, first, share, 7)

    if parked and not first:
        assert got is None and not calls
        assert cell.buf is buf                                          # a share in the buffer stays where it is ...
        assert len(cell.take_dicts()) == n_items                        # ... and the parked ones wait for the first reader
        return
    want = (0.0 if parked else SHARE) + (MULTI if (first and n_items) else 0.0) + (BUF if has_buf else 0.0)
    assert len(calls) == (1 if (first and n_items) else 0)
    if calls:
        assert calls[0][1] == 7 and [it[0][1] for it in calls[0][0]] == list(range(n_items))
    total = got if first else cell.buf
    assert torch.equal(total, _t(want)), (total, want)                  # every addend once, none twice
    if first:
        assert cell.buf is None and cell.take_dicts() == []             # the total went to autograd: the cell is clear
    else:
        assert got is None
        assert len(cell.take_dicts()) == n_items                        # only the first reader runs the multi launch


def test_settle_without_a_cell_returns_the_share():
    from kp_gnn_amd import ops
    g = _t(SHARE)
    assert ops._settle_dict_share(None, False, ops._DictShare(g), 7) is g


def test_unpark_takes_back_the_last_parked_share():
    from kp_gnn_amd import ops
    cell = ops._SlotGradCell()
    cell.park_dict("u0", "t0", "g0")
    cell.park_dict("u1", "t1", "g1")
    cell.unpark_dict()
    assert cell.take_dicts() == [("u0", "t0", "g0")] and cell.take_dicts() == []
