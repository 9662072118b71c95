"""pfn_eval_metrics / pfn_eval_accumulate (csrc/eval.hip) through the C ABI.  Yardstick: this package's MaskedL2V2 / MaskedL1 and
oracle.ref_cpu.masked_l2_loss evaluated in float64 on the CPU from the kernel's own fp32 inputs, de-normalised the reference's way
(out * std + mean and y * std + mean, then the metric).  Bound: every term within tests/util.RTOL of the float64 value, term by
term; exact zeros and the NaN pattern are held to equality; the running sums are held to the bits of the host loop."""
import ctypes as C
import math

import pytest
import torch

from oracle import ref_cpu
from poweflownet_amd import _lib as L
from poweflownet_amd.utils.custom_loss_functions import MaskedL1, MaskedL2V2
from tests.util import RTOL, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NT = len(L.EVAL_TERMS)
GUARD = 12345.0
ROWS = (0, 1, 3, 255, 256, 257, 1652, 65536, 65537, 70001)      # ... the 256-block x 256-row cap and one row past it
STD = (0.05, 10.0, 50.0, 20.0)
MEAN = (1.0, 0.0, 30.0, 10.0)
BUS_TABLE = torch.tensor([[0, 0, 1, 1], [0, 1, 0, 1], [1, 1, 0, 0]], dtype=torch.int64)     # slack / PV / PQ: what is predicted


def _stream():
    return torch.cuda.current_stream().cuda_stream


def make_inputs(n, kind, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + n)
    o = torch.randn(n, 4, generator=g)
    y = o + 0.1 * torch.randn(n, 4, generator=g)
    x = torch.randn(n, 4, generator=g)
    if kind == "bus":
        m = BUS_TABLE[torch.randint(0, 3, (n,), generator=g)]
    elif kind == "frac":
        m = torch.randint(0, 5, (n, 4), generator=g).float() * 0.25           # 0, .25, .5, .75, 1: 1 - m is exact in fp32
    elif kind == "zero_col":
        m = torch.randint(0, 2, (n, 4), generator=g)
        m[:, 2] = 0
    else:
        m = torch.zeros(n, 4, dtype=torch.int64)
    return o, y, x, m


def reference(o, y, m, std):
    """{term name: float64 value} from the fp32 inputs."""
    o64, y64 = o.double(), y.double()
    m64 = m if m.dtype == torch.int64 else m.double()
    ref = {}
    for f, name in enumerate(("vm", "va", "p", "q")):
        ref[f"cnt_{name}"] = float(m64[:, f].sum())
    s64 = torch.tensor(STD if std else (1.0,) * 4, dtype=torch.float32).double()
    mean64 = torch.tensor(MEAN if std else (0.0,) * 4, dtype=torch.float64)
    for fam, loss, a, b in (("l2", MaskedL2V2(), o64, y64), ("l1", MaskedL1(), o64, y64),
                            ("l2d", MaskedL2V2(), o64 * s64 + mean64, y64 * s64 + mean64),
                            ("l1d", MaskedL1(), o64 * s64 + mean64, y64 * s64 + mean64)):
        for k, v in loss(a, b, m64).items():
            ref[f"{fam}_{'balanced' if k == 'balanced total' else k}"] = float(v)
    ref["ml2_selected"] = float(ref_cpu.masked_l2_loss(o64, y64, m64, regularize=False))
    ref["ml2_regularizer"] = float(ref_cpu.masked_l2_loss(o64, y64, 1 - m64, regularize=False))
    ref["mse"] = float(((o64 - y64) ** 2).mean()) if o.numel() else float("nan")
    assert tuple(ref) != () and set(ref) == set(L.EVAL_TERMS)
    return ref


class Launch:
    """One call through the C ABI with guard floats around every output."""

    def __init__(self, n, with_x, with_acc):
        self.n = n
        self.tbuf = torch.full((NT + 16,), GUARD, device=DEV)
        self.terms = self.tbuf[8:8 + NT]
        self.mbuf = torch.full((n + 2, 4), GUARD, device=DEV) if with_x else None
        self.mixed = self.mbuf[1:n + 1] if with_x else None
        self.abuf = torch.full((L.EVAL_ACC_DOUBLES + 2,), GUARD, dtype=torch.float64, device=DEV) if with_acc else None
        self.acc = self.abuf[1:1 + L.EVAL_ACC_DOUBLES] if with_acc else None
        if with_acc:
            self.acc.zero_()
        self.ws = torch.zeros(L.EVAL_WS_FLOATS, device=DEV)

    def __call__(self, o, y, x, m, std, weight=1.0, first_unweighted=False):
        st = (C.c_float * 4)(*STD) if std else None
        L.check(L.load().pfn_eval_metrics(o.data_ptr(), y.data_ptr(), L.ptr(x) if self.mixed is not None else None, m.data_ptr(),
                                          0 if m.dtype == torch.int64 else 1, o.shape[0], st, float(weight), int(first_unweighted),
                                          self.terms.data_ptr(), L.ptr(self.acc), L.ptr(self.mixed), self.ws.data_ptr(),
                                          self.ws.numel() * 4, _stream()), "pfn_eval_metrics")
        return self.terms.cpu()

    def check_guards(self):
        assert (self.tbuf[:8] == GUARD).all() and (self.tbuf[8 + NT:] == GUARD).all(), "terms: a guard float was written"
        if self.mbuf is not None:
            assert (self.mbuf[0] == GUARD).all() and (self.mbuf[-1] == GUARD).all(), "mixed_out: a guard row was written"
        if self.abuf is not None:
            assert self.abuf[0] == GUARD and self.abuf[-1] == GUARD, "epoch_acc: a guard double was written"
        assert int(self.ws.view(torch.int32)[6656]) == 0, "the arrival counter was not re-armed"


def assert_terms(got, ref, what):
    worst = 0.0
    for i, name in enumerate(L.EVAL_TERMS):
        g, r = float(got[i]), ref[name]
        if math.isnan(r):
            assert math.isnan(g), f"{what}: {name} = {g}, float64 gives NaN"
        elif r == 0.0:
            assert g == 0.0, f"{what}: {name} = {g}, float64 gives exactly 0"
        else:
            assert not math.isnan(g), f"{what}: {name} is NaN, float64 gives {r}"
            rel = abs(g - r) / abs(r)
            worst = max(worst, rel)
            assert rel <= RTOL, f"{what}: {name} = {g!r}, float64 {r!r}: {rel:.2e} relative, bound {RTOL:g}"
    record(f"{what}: worst term", worst, 1.0, RTOL)
    return worst


@pytest.mark.parametrize("kind", ["bus", "frac", "zero_col", "all_zero"])
@pytest.mark.parametrize("n", ROWS)
def test_terms_against_float64(n, kind):
    o, y, x, m = make_inputs(n, kind)
    do, dy, dx, dm = (t.to(DEV) for t in (o, y, x, m))
    for std, with_x in ((False, False), (True, True)):
        run = Launch(n, with_x, with_acc=False)
        got = run(do, dy, dx, dm, std)
        run.check_guards()
        ref = reference(o, y, m, std)
        worst = assert_terms(got, ref, f"n={n} {kind} std={std}")
        print(f"n={n} {kind} std={std}: worst relative error {worst:.3e}")
        if with_x:
            want = o * m + x * (1 - m)
            assert torch.equal(run.mixed.cpu(), want), "mixed_out differs from out * mask + x * (1 - mask)"
    if kind == "zero_col" and n > 0:
        assert ref["l2_p"] == 0.0 and ref["cnt_p"] == 0.0                     # the clamp: the test above held the term to exactly 0
    if kind == "all_zero":
        assert math.isnan(ref["ml2_selected"]) and ref["l2_total"] == 0.0 and ref["l1d_balanced"] == 0.0


@pytest.mark.parametrize("kind", ["bus", "frac"])
@pytest.mark.parametrize("n", [257, 1652])
def test_nan_pattern(n, kind):
    """A NaN under a ZERO mask entry poisons its column (the mask multiplies), one under a non-zero entry does too; which terms
    turn NaN is what float64 says."""
    o, y, x, m = make_inputs(n, kind, seed=1)
    for want_zero in (True, False):
        o2 = o.clone()
        rows = ((m[:, 1] == 0) if want_zero else (m[:, 1] != 0)).nonzero().flatten()
        r = int(rows[len(rows) // 2])
        o2[r, 1] = float("nan")
        run = Launch(n, True, with_acc=False)
        got = run(o2.to(DEV), y.to(DEV), x.to(DEV), m.to(DEV), True)
        run.check_guards()
        ref = reference(o2, y, m, True)
        assert math.isnan(ref["l2_va"]) and math.isnan(ref["mse"]) and not math.isnan(ref["l2_vm"])
        assert math.isnan(ref["ml2_selected"]) == (not want_zero)
        assert_terms(got, ref, f"nan under {'zero' if want_zero else 'non-zero'} mask, n={n} {kind}")


def _host_loop(term_rows, weights, first_unweighted):
    acc = [0.0] * NT
    for b, (terms, w) in enumerate(zip(term_rows, weights)):
        wt = 1.0 if (first_unweighted and b == 0) else w
        for k in range(NT):
            acc[k] += float(terms[k]) * wt
    return acc


def _same_doubles(a, b):
    return all((math.isnan(p) and math.isnan(q)) or p == q for p, q in zip(a, b))


@pytest.mark.parametrize("first_unweighted", [False, True])
def test_epoch_accumulators_equal_the_host_loop(first_unweighted):
    sizes, weights = (1652, 1652, 826), (8.0, 7.0, 3.0)         # (not all powers of two: a fused multiply-add would show)
    batches = [tuple(t.to(DEV) for t in make_inputs(n, "bus", seed=10 + i)) for i, n in enumerate(sizes)]
    run = Launch(max(sizes), False, with_acc=True)
    for round_ in range(2):                                                   # ... then cleared and run again
        rows = [run(o, y, x, m, True, w, first_unweighted).clone() for (o, y, x, m), w in zip(batches, weights)]
        got = run.acc.cpu()
        assert int(got[NT:].view(torch.int64)[0]) == 3
        want = _host_loop(rows, weights, first_unweighted)
        assert _same_doubles(got[:NT].tolist(), want), (round_, got[:NT].tolist(), want)
        run.check_guards()
        run.acc.zero_()
    # pfn_eval_accumulate: acc[0] += double(loss) * w, the first batch unweighted on request
    lib = L.load()
    abuf = torch.full((4,), GUARD, dtype=torch.float64, device=DEV)
    acc = abuf[1:3]
    acc.zero_()
    losses = torch.tensor([0.1234567, 3.25e-5, 7.0e3], device=DEV)
    for i, w in enumerate((7.0, 8.0, 6.0)):
        L.check(lib.pfn_eval_accumulate(losses[i:i + 1].data_ptr(), w, int(first_unweighted), acc.data_ptr(), _stream()), "acc")
    want = 0.0
    for i, w in enumerate((7.0, 8.0, 6.0)):
        want += float(losses[i].item()) * (1.0 if (first_unweighted and i == 0) else w)
    got = abuf.cpu()
    assert float(got[1]) == want and int(got[2:3].view(torch.int64)[0]) == 3 and got[0] == GUARD and got[3] == GUARD


def test_replay_from_a_graph_gives_the_bits_of_eager_calls():
    """The launch captured in a torch.cuda.graph and replayed three times over changed inputs == three eager calls: the ticket
    is re-armed by every launch and no partial of an earlier one survives."""
    from poweflownet_amd.loss import _Workspace, eval_accumulator, eval_metrics
    n = 70001                                                                 # 256 blocks, a second row for some threads
    sets = [tuple(t.to(DEV) for t in make_inputs(n, "frac", seed=20 + i)) for i in range(3)]
    eager_terms, acc_e, ws_e = [], eval_accumulator(DEV, 1, L.EVAL_ACC_DOUBLES).view(-1), _Workspace(L.EVAL_WS_FLOATS)
    eager_mixed = []
    for o, y, x, m in sets:
        mixed = torch.empty_like(o)
        eager_terms.append(eval_metrics(o, y, m, x=x, std=STD, weight=7.0, first_unweighted=True, acc=acc_e, mixed_out=mixed,
                                        workspace=ws_e).clone())
        eager_mixed.append(mixed)
    so, sy, sx, sm = (t.clone() for t in sets[0])
    acc_g, ws_g = eval_accumulator(DEV, 1, L.EVAL_ACC_DOUBLES).view(-1), _Workspace(L.EVAL_WS_FLOATS)
    terms_g, mixed_g = torch.empty(NT, device=DEV), torch.empty_like(so)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eval_metrics(so, sy, sm, x=sx, std=STD, weight=7.0, first_unweighted=True, acc=acc_g, mixed_out=mixed_g, terms=terms_g,
                     workspace=ws_g)
    torch.cuda.current_stream().wait_stream(side)
    acc_g.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eval_metrics(so, sy, sm, x=sx, std=STD, weight=7.0, first_unweighted=True, acc=acc_g, mixed_out=mixed_g, terms=terms_g,
                     workspace=ws_g)
    for i, (o, y, x, m) in enumerate(sets):
        for dst, src in ((so, o), (sy, y), (sx, x), (sm, m)):
            dst.copy_(src)
        g.replay()
        assert torch.equal(terms_g.view(torch.int32), eager_terms[i].view(torch.int32)), f"replay {i}: terms differ from the eager call"
        assert torch.equal(mixed_g, eager_mixed[i])
    assert torch.equal(acc_g.view(torch.int64), acc_e.view(torch.int64))
    assert int(acc_g[NT:].view(torch.int64)[0]) == 3


def test_argument_errors():
    lib = L.load()
    t = torch.zeros(8, 4, device=DEV)
    terms, ws = torch.zeros(NT, device=DEV), torch.zeros(L.EVAL_WS_FLOATS, device=DEV)
    rc = lib.pfn_eval_metrics(t.data_ptr(), t.data_ptr(), None, t.data_ptr(), 1, 8, None, 1.0, 0, terms.data_ptr(), None,
                              t.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream())
    assert rc == -1 and b"mixed_out needs x" in lib.pfn_last_error()
    rc = lib.pfn_eval_metrics(t.data_ptr(), t.data_ptr(), None, t.data_ptr(), 1, 8, None, 1.0, 0, terms.data_ptr(), None, None,
                              ws.data_ptr(), 64, _stream())
    assert rc != 0 and b"workspace too small" in lib.pfn_last_error()
    rc = lib.pfn_eval_metrics(t.data_ptr() + 4, t.data_ptr(), None, t.data_ptr(), 1, 7, None, 1.0, 0, terms.data_ptr(), None, None,
                              ws.data_ptr(), ws.numel() * 4, _stream())
    assert rc == -1 and b"16-byte aligned" in lib.pfn_last_error()
