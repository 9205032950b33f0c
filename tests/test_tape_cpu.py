"""The summation and ordering contract of vsr_amd/nets/tape.py, on the host:
functional.add is replaced by a function that records which operands it was
given, so the grouping of every sum is read off, not inferred from values.

* Bwd keeps a tensor's gradient contributions apart and folds from the tail:
  arrivals a, b, c give take_list(t, 2) = [a, b + c] and take(t) = a + (b + c);
  one contribution comes back as it is, without an add.
* EDVRNet's subclass sums on arrival: (a + b) + c, the adds inside acc.
* route with parts delivers channel slices to the part tensors and nothing to
  the concat buffer.
* ParamGrads.buf reports seen False once, then True; done() hands the
  parameters over in first-touch order.
"""
import pytest
import torch

from vsr_amd import functional
from vsr_amd.nets import tape
from vsr_amd.nets.edvr_net import _Bwd as EDVRBwd


class StubNet:
    compute_dtype = torch.float32

    def __init__(self):
        self.handed = []

    def _grad_buffer(self, p):
        return torch.empty_like(p, dtype=torch.float32)

    def _grad_done(self, out, p, g):
        self.handed.append(p)
        out[id(p)] = g

    def _const(self, dev, value):
        return torch.full((1,), value, dtype=torch.float32, device=dev)


class Adds:
    """Host stand-in for functional.add: names every tensor by how it was made."""

    def __init__(self, **named):
        self.names = {id(t): n for n, t in named.items()}
        self.keep = list(named.values())  # ids stay unique while the tensors live
        self.calls = []

    def __call__(self, a, b, out):
        out.copy_(a + b)
        name = f"({self.names[id(a)]}+{self.names[id(b)]})"
        self.names[id(out)] = name
        self.keep.append(out)
        self.calls.append(name)
        return out

    def name(self, t):
        return self.names[id(t)]


def view(value):
    return torch.full((1, 1, 2, 3, 4), float(value))


@pytest.fixture
def abc(monkeypatch):
    a, b, c = view(1), view(10), view(100)
    adds = Adds(a=a, b=b, c=c)
    monkeypatch.setattr(functional, "add", adds)
    return a, b, c, adds


def test_base_take_list_folds_from_the_tail(abc):
    a, b, c, adds = abc
    bk = tape.Bwd(StubNet())
    t = view(0)
    for g in (a, b, c):
        bk.acc(t, g)
    assert adds.calls == []  # nothing is summed on arrival
    got = bk.take_list(t, 2)
    assert [adds.name(g) for g in got] == ["a", "(b+c)"] and got[0] is a
    assert adds.calls == ["(b+c)"]
    assert torch.equal(got[1], view(110))
    assert id(t) not in bk.G


def test_base_take_groups_a_plus_b_plus_c(abc):
    a, b, c, adds = abc
    bk = tape.Bwd(StubNet())
    t = view(0)
    for g in (a, b, c):
        bk.acc(t, g)
    got = bk.take(t)
    assert adds.name(got) == "(a+(b+c))"
    assert adds.calls == ["(b+c)", "(a+(b+c))"]
    assert torch.equal(got, view(111))


def test_one_contribution_comes_back_without_an_add(abc):
    a, _, _, adds = abc
    for bk in (tape.Bwd(StubNet()), EDVRBwd(StubNet(), dev=torch.device("cpu"), pk={}, sp=None)):
        t = view(0)
        bk.acc(t, a)
        assert bk.take(t) is a
    assert adds.calls == []


def test_edvr_sums_on_arrival_left_to_right(abc):
    a, b, c, adds = abc
    bk = EDVRBwd(StubNet(), dev=torch.device("cpu"), pk={}, sp=None)
    t = view(0)
    bk.acc(t, a)
    assert adds.calls == []
    bk.acc(t, b)
    assert adds.calls == ["(a+b)"]  # inside acc, at arrival
    bk.acc(t, c)
    assert adds.calls == ["(a+b)", "((a+b)+c)"]
    assert len(bk.G[id(t)]) == 1  # never more than one held
    got = bk.take(t)
    assert adds.name(got) == "((a+b)+c)" and adds.calls == ["(a+b)", "((a+b)+c)"]
    assert torch.equal(got, view(111))


@pytest.mark.parametrize("make", [lambda: tape.Bwd(StubNet()),
                                  lambda: EDVRBwd(StubNet(), dev=torch.device("cpu"), pk={}, sp=None)], ids=["base", "edvr"])
def test_route_delivers_channel_slices_to_the_parts(abc, make):
    _, _, _, adds = abc
    bk = make()
    cat = torch.zeros((1, 1, 2, 3, 6))
    lo, hi = cat[..., :2], cat[..., 2:]
    gx = torch.arange(36, dtype=torch.float32).view(1, 1, 2, 3, 6)
    bk.route(cat, [(lo, 0, 2), (hi, 2, 6)], gx)
    assert id(cat) not in bk.G
    assert torch.equal(bk.take(lo), gx[..., 0:2]) and torch.equal(bk.take(hi), gx[..., 2:6])
    bk.route(cat, None, gx)  # no parts: the tensor itself
    assert bk.take(cat) is gx
    assert adds.calls == [] and bk.G == {}


def test_run_seeds_and_runs_the_ops_last_to_first(abc):
    a, _, _, _ = abc
    net = StubNet()
    bk = tape.Bwd(net)
    yv, mid = view(0), view(0)
    p = torch.nn.Parameter(torch.zeros(2))
    order = []

    def first(bk_):
        order.append("first")
        assert bk_.take(mid) is a
        bk_.buf(p)

    def last(bk_):
        order.append("last")
        bk_.acc(mid, bk_.take(yv))

    out = bk.run([first, last], yv, a)
    assert order == ["last", "first"] and list(out) == [id(p)] and bk.G == {}


def test_param_grads_seen_flag_and_first_touch_order():
    net = StubNet()
    pg = tape.ParamGrads(net)
    p, q, r = (torch.nn.Parameter(torch.zeros(n)) for n in (2, 3, 4))
    gq, seen = pg.buf(q)
    assert seen is False and gq.dtype == torch.float32 and gq.shape == q.shape
    assert pg.buf(p)[1] is False
    again, seen = pg.buf(q)
    assert seen is True and again is gq
    assert pg.buf(r)[1] is False and pg.buf(p)[1] is True
    assert net.handed == []
    out = pg.done()
    assert [id(x) for x in net.handed] == [id(q), id(p), id(r)]
    assert list(out) == [id(q), id(p), id(r)] and out[id(q)] is gq


def test_storage_helpers():
    assert [tape.cp(c) for c in (1, 8, 9, 64)] == [8, 8, 16, 64]
    v = tape.empty_view((2, 1, 3, 5), 3, torch.float32, torch.device("cpu"), zero=True)
    assert v.shape == (2, 1, 3, 5, 3) and v.stride() == (120, 120, 40, 8, 1) and not v.any()
    ops, push = tape.recorder(False)
    push(len)
    assert ops is None
    ops, push = tape.recorder(True)
    push(len)
    assert ops == [len]
