"""The small kernels around a training step against float64 references (-m gpu): `adamw_kernel` (csrc/util_kernels.hip) through
its three C entry points and through `FlatAdamW`, `power_imbalance_fwd_kernel` (csrc/physics.hip) above its 256-block cap, and
`mse_kernel` / `masked_l2_reduce_kernel` at the element counts where their block count changes.

AdamW yardstick: `oracle.ref_cpu.adamw_step`, float64, which tests/test_oracle.py pins to torch.optim.AdamW run in float64.  A single
update is launched from an INJECTED state (parameters, gradient, both moments and the device step counter preset), so every value of
{size, alignment, step number, hyper-parameters, fresh / warm state} is reached directly instead of through a training run:

  * the reference is fed the kernel's own fp32 inputs and the hyper-parameters as the C ABI carries them (fp32, widened); the
    distance to the same update with the true Python doubles -- what torch.optim.AdamW computes with -- is recorded only
    (tests/util.record): it is the rounding of 0.999 and friends to fp32, a property of the interface;
  * `exp_avg` / `exp_avg_sq`: tests/util.assert_close, 1e-5 of the largest entry (the project's own tolerance);
  * parameters: the UPDATE p_new - p_old is compared, normwise (max |error| <= UPDATE_RTOL * max |reference update|) -- an error in
    a 1e-3 update disappears in p's own magnitude.  What an fp32 evaluation of the formula can reach under this measure was
    measured on the CPU with torch.optim.AdamW itself (fp32, foreach=False, the same injected states and the same widened
    hyper-parameters; every case the tests below run) against the same float64 reference.  Nearly all of it is the rounding of
    p_new to fp32 -- parameters are uniform in +-0.1, the range of this model's Linear initialisation (1 / sqrt(129) = 0.088), so
    half an ulp of p is up to 3.7e-9, against an update of about lr:
        torch defaults, 262,149 elements, t = 1 (fresh / warm) / 2 / 3 / 10 / 1000 / 100001
                                            8.78e-6 / 7.23e-6 / 9.82e-6 / 1.14e-5 / 1.51e-5 / 2.91e-6 / 2.33e-6
        t = 10, 1023 .. 786,437 elements                        1.51e-5 .. 1.80e-5
        t = 10, 1 / 3 / 4 / 5 elements                          3.31e-6 / 3.71e-5 / 1.03e-5 / 4.35e-5  (a handful of updates: a small scale)
        OneCycleLR at its peak (lr 1e-3, beta1 0.85)            1.78e-5 (262,149) / 1.99e-5 (1025, scalar path) / 8.06e-6 (fresh)
        weight_decay 0                                          6.56e-6 / 7.12e-6 / 3.79e-6
        weight_decay 0.1                                        1.55e-5 / 1.65e-5 / 7.60e-6
        eps 1e-3                                                1.53e-5 / 1.63e-5 / 7.85e-6
        beta2 0.99                                              5.43e-6 / 5.72e-6 / 8.06e-6
        beta1 0                                                 1.34e-5 / 1.51e-5 / 8.06e-6
        OneCycleLR at its start (lr 4e-5, beta1 0.95)           2.53e-4 / 2.57e-4 / 2.16e-4   (the update is 25 x smaller, p's ulp is not)
    The bound is 4 x the reference's worst error, the factor tests/util._check_full_size allows between two fp32 evaluation orders
    of one function, per learning rate (the one axis that moves the reference error by an order of magnitude):
        UPDATE_RTOL[lr 1e-3] = 4 x 4.35e-5 = 1.74e-4,    UPDATE_RTOL[lr 4e-5] = 4 x 2.57e-4 = 1.03e-3
    In the block of exact zeros (g = m = v = 0) the update is the decay -lr wd p alone and the moments stay 0.  Its only roundings are
    those of 1 - lr wd and of the product, 2^-24 |p| each: the block's update is held to 2^-23 of its largest |p| (the decay itself is
    84 x that at torch's defaults, 3.4 x at lr 4e-5).

Trajectory (300 steps under OneCycleLR, test_flat_adamw_follows_onecycle_for_300_steps): float64 torch.optim.AdamW on the CPU, fed
the same gradients, open loop.  Measure: max |p_k - ref_k| over max |ref_k - p_0|, the displacement since the start.  The fp32
torch.optim.AdamW CPU trajectory under that measure, and 4 x it (TRAJ_RTOL):
        after step 1: 6.08e-4 -> 2.43e-3     step 10: 3.50e-4 -> 1.40e-3     step 100: 8.33e-6 -> 3.33e-5     step 300: 5.23e-6 -> 2.09e-5
(the first steps run at lr 4e-5: a displacement of 4e-5 against the same half ulp of p).
"""
import copy
import functools

import pytest
import torch

from oracle import ref_cpu
from tests.util import RTOL, assert_close, record, record_elementwise, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ------------------------------------------------------------------------------------------------ AdamW: cases
# 4 x the error of torch.optim.AdamW (fp32, CPU, foreach=False) against ref_cpu.adamw_step on the same injected states, normwise on
# the update, keyed by the learning rate: measured 4.35e-5 at lr 1e-3 (the worst of every case run below: 5 elements; 2.0e-5 from
# 1023 elements on), 2.57e-4 at lr 4e-5 (table in the module docstring; the measurement itself: torch32_update_error below)
UPDATE_RTOL = {1e-3: 1.74e-4, 4e-5: 1.03e-3}
# 4 x the error of the fp32 torch.optim.AdamW CPU trajectory against the float64 one, max |p_k - ref_k| / max |ref_k - p_0|:
# measured 6.08e-4 / 3.50e-4 / 8.33e-6 / 5.23e-6 after steps 1 / 10 / 100 / 300 (torch_cpu_trajectory(torch.float32) below)
TRAJ_RTOL = {1: 2.43e-3, 10: 1.40e-3, 100: 3.33e-5, 300: 2.09e-5}

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 262_143, 262_144, 262_149, 786_437]   # 262,144 = 256 blocks x 256 lanes x 4: one full trip
ALIGNMENTS = {"aligned": (0, 0, 0, 0), "p+1": (1, 0, 0, 0), "g+1": (0, 1, 0, 0), "m+1": (0, 0, 1, 0), "v+1": (0, 0, 0, 1),
              "all+1": (1, 1, 1, 1)}                                          # offset, in floats, of (p, g, m, v)
STEPS_BEFORE = [0, 1, 2, 9, 999, 100_000]
DEFAULTS = (1e-3, 0.9, 0.999, 1e-8, 1e-2)                                     # lr, beta1, beta2, eps, weight_decay (torch's)
HYPERS = {
    "defaults": DEFAULTS,
    "onecycle start": (1e-3 / 25, 0.95, 0.999, 1e-8, 1e-2),                   # OneCycleLR(max_lr=1e-3): lr max_lr / 25, beta1 0.95
    "onecycle peak": (1e-3, 0.85, 0.999, 1e-8, 1e-2),
    "weight_decay 0": (1e-3, 0.9, 0.999, 1e-8, 0.0),
    "weight_decay 0.1": (1e-3, 0.9, 0.999, 1e-8, 0.1),
    "eps 1e-3": (1e-3, 0.9, 0.999, 1e-3, 1e-2),
    "beta2 0.99": (1e-3, 0.9, 0.99, 1e-8, 1e-2),
    "beta1 0": (1e-3, 0.0, 0.999, 1e-8, 1e-2),
}
N_AXIS = 262_149          # the size the one-axis-at-a-time cases run at: two trips of the float4 loop and a one-element tail
T_AXIS = 9                # ... and their step counter before the call
SENTINEL = -1234.5
PAD = 8                   # floats checked in front of and behind every array
SKIPPED = 7               # preset step_count[2]: an unguarded or finite-guard launch must leave it alone


def widened(hyper):
    """The five scalars as the C ABI carries them: rounded to fp32, as Python floats."""
    return tuple(torch.tensor(hyper, dtype=torch.float32).double().tolist())


def update_rtol(hyper):
    return UPDATE_RTOL[1e-3 if hyper[0] > 5e-4 else 4e-5]


@functools.lru_cache(maxsize=None)
def make_state(n, warm=True, seed=0):
    """(p, g, m, v), fp32 on the CPU, never modified.  Gradient magnitudes log-uniform over 1e-8 .. 1e2 with random signs; a warm
    state holds the moments of earlier gradients of each entry's own magnitude; a fresh one zeros.  From 64 elements on, a block of
    37 entries (starting at an odd index, so it straddles float4 groups) has g = m = v = 0 exactly."""
    gen = torch.Generator().manual_seed(1000 * seed + n % 997 + (5 if warm else 0))
    p = 0.1 * (2.0 * torch.rand(n, generator=gen) - 1.0)
    mag = 10.0 ** (torch.rand(n, generator=gen) * 10.0 - 8.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g = mag * sign * (0.5 + torch.rand(n, generator=gen))
    if warm:
        m = mag * sign * (0.2 + 0.6 * torch.rand(n, generator=gen)) * torch.where(torch.rand(n, generator=gen) < 0.2, -1.0, 1.0)
        v = mag * mag * (0.05 + torch.rand(n, generator=gen))
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    z = zero_block(n)
    g[z], m[z], v[z] = 0.0, 0.0, 0.0
    return tuple(t.float().contiguous() for t in (p, g, m, v))


def zero_block(n):
    return slice(n // 3 | 1, (n // 3 | 1) + 37) if n >= 64 else slice(0, 0)


@functools.lru_cache(maxsize=None)
def reference(n, warm, t_before, hyper, seed=0):
    """float64 (p, m, v) after the update number t_before + 1, hyper-parameters as given."""
    return ref_cpu.adamw_step(*make_state(n, warm, seed), t_before + 1, *hyper)


def torch32_update_error(n, warm, t_before, hyper, seed=0):
    """The measurement behind UPDATE_RTOL: torch.optim.AdamW in fp32 on the CPU from the same injected state, its update against
    the float64 reference under the measure the kernel is held to.  Returns (error, scale)."""
    p, g, m, v = make_state(n, warm, seed)
    h = widened(hyper)
    w = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([w], lr=h[0], betas=(h[1], h[2]), eps=h[3], weight_decay=h[4], foreach=False)
    opt.state[w].update(step=torch.tensor(float(t_before)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    w.grad = g.clone()
    opt.step()
    return rel_err(w.detach().double() - p.double(), reference(n, warm, t_before, h, seed)[0] - p.double())


# ------------------------------------------------------------------------------------------------ AdamW: launching
def _carve(host, offset):
    """A device copy of `host` inside a larger buffer filled with SENTINEL, `offset` floats past a 16-byte boundary."""
    n = host.numel()
    buf = torch.full((PAD + offset + n + PAD + 4,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + offset:PAD + offset + n]
    view.copy_(host)
    return buf, view


def _sentinels_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    n = view.numel()
    s = torch.tensor(SENTINEL)
    return bool((buf[lo - PAD:lo] == s).all().item()) and bool((buf[lo + n:lo + n + PAD] == s).all().item())


def launch(entry, state, t_before, hyper, align=(0, 0, 0, 0), guard=None, skipped=SKIPPED):
    """One launch of `entry` ("dev", "value", "guarded") from the injected state.  Returns p, m, v (CPU), the step counter as a list
    and the guard-free invariants checked here: the gradient and the 8 floats around all four arrays are untouched."""
    from poweflownet_amd import _lib as L
    lib = L.load()
    bufs = [_carve(t, o) for t, o in zip(state, align)]
    (_, p), (_, g), (_, m), (_, v) = bufs
    for (_, view), o in zip(bufs, align):
        assert view.data_ptr() % 16 == 4 * o
    n = p.numel()
    step = torch.tensor([t_before, 0, skipped], dtype=torch.int64, device=DEV)
    hp = torch.tensor(hyper, dtype=torch.float32, device=DEV)
    if entry == "dev":
        rc = lib.pfn_adamw_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hp.data_ptr(), step.data_ptr(),
                                    L.stream_ptr())
    elif entry == "value":
        rc = lib.pfn_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *hyper, step.data_ptr(), L.stream_ptr())
    else:
        gd = torch.tensor([guard], dtype=torch.float32, device=DEV)
        rc = lib.pfn_adamw_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hp.data_ptr(), step.data_ptr(),
                                        gd.data_ptr(), L.stream_ptr())
    L.check(rc, f"pfn_adamw_step ({entry})")
    torch.cuda.synchronize()
    for name, (buf, view) in zip("pgmv", bufs):
        assert _sentinels_intact(buf, view), f"{name}: the floats around the array were written (n {n}, offsets {align})"
    assert torch.equal(g.cpu(), state[1]), "the gradient was written"
    return p.cpu(), m.cpu(), v.cpu(), step.tolist()


def check_update(what, n, warm, t_before, hyper, align=(0, 0, 0, 0), entries=("dev", "value")):
    """Section 2 of the module docstring for one case, through pfn_adamw_step_dev and pfn_adamw_step."""
    state = make_state(n, warm)
    p0 = state[0].double()
    h32 = widened(hyper)
    p_ref, m_ref, v_ref = reference(n, warm, t_before, h32)
    got = {}
    for entry in entries:
        p, m, v, step = launch(entry, state, t_before, hyper, align)
        got[entry] = (p, m, v)
        w = f"{what} [{entry}]"
        assert step == [t_before + 1, 0, SKIPPED], (w, step)
        assert_close(m, m_ref.float(), RTOL, f"{w}: exp_avg")
        assert_close(v, v_ref.float(), RTOL, f"{w}: exp_avg_sq")
        record_elementwise(m, m_ref, f"{w}: exp_avg")
        record_elementwise(v, v_ref, f"{w}: exp_avg_sq")
        bound = update_rtol(hyper)
        err, scale = rel_err(p.double() - p0, p_ref - p0)
        record(f"{w}: update vs fp64 (fp32 hyper-parameters widened)", err, scale, bound)
        assert err <= bound * scale, f"{w}: update error {err:.3e} = {err / scale:.2e} of the largest update {scale:.3e}, bound {bound:g}"
        z = zero_block(n)
        if z.stop > z.start:
            # g = m = v = 0: the moments stay exactly 0 and the update is the decay alone
            assert not m[z].any() and not v[z].any(), w
            err, scale = rel_err(p[z].double() - p0[z], p_ref[z] - p0[z])
            record(f"{w}: decay-only block", err, scale, None)
            if h32[4] == 0.0:
                assert torch.equal(p[z], state[0][z]), w
            else:
                pmax = state[0][z].abs().max().item()
                assert err <= 2.0 ** -23 * pmax, f"{w}: decay-only block: error {err:.3e}, decay {scale:.3e}, 2^-23 max|p| {2.0 ** -23 * pmax:.3e}"
        d_ref = reference(n, warm, t_before, tuple(float(x) for x in hyper))[0] - p0
        err, scale = rel_err(p.double() - p0, d_ref)
        record(f"{w}: update vs fp64 with the Python-double hyper-parameters (recorded only)", err, scale, None)
    if len(entries) == 2:
        for a, b, name in zip(got["dev"], got["value"], ("p", "exp_avg", "exp_avg_sq")):
            assert torch.equal(a, b), f"{what}: {name} differs between pfn_adamw_step_dev and pfn_adamw_step"


# ------------------------------------------------------------------------------------------------ AdamW: single update
@pytest.mark.parametrize("n", SIZES)
def test_adamw_update_every_size_and_alignment(n):
    """The full size x alignment grid at torch's defaults, warm state, 10th update: the float4 path (all four arrays 16-byte
    aligned), the scalar path (any one of them, or all, one float off), the n % 4 tail, one / two / three trips of the grid-stride
    loop."""
    for name, align in ALIGNMENTS.items():
        check_update(f"n {n}, {name}", n, True, T_AXIS, DEFAULTS, align)


@pytest.mark.parametrize("t_before", STEPS_BEFORE)
def test_adamw_update_every_step_number(t_before):
    """The bias corrections 1 - beta^t at t = 1, 2, 3, 10, 1000 and 100,001 (fp32 powf on the device); t = 1 from a fresh state
    (m = v = 0) and, like every other, from a warm one."""
    for warm in ((False, True) if t_before == 0 else (True,)):
        check_update(f"t {t_before} -> {t_before + 1}, {'warm' if warm else 'fresh'}", N_AXIS, warm, t_before, DEFAULTS)


@pytest.mark.parametrize("name", list(HYPERS))
def test_adamw_update_every_hyper_parameter(name):
    """Each hyper-parameter away from torch's default in turn, read from the device (pfn_adamw_step_dev) and passed by value
    (pfn_adamw_step): OneCycleLR's two extremes, weight_decay 0 and 0.1, eps 1e-3, beta2 0.99, beta1 0; on both code paths."""
    check_update(f"{name}, aligned", N_AXIS, True, T_AXIS, HYPERS[name])
    check_update(f"{name}, scalar path", 1025, True, T_AXIS, HYPERS[name], ALIGNMENTS["g+1"])
    check_update(f"{name}, fresh, first update", 1027, False, 0, HYPERS[name])


# ------------------------------------------------------------------------------------------------ AdamW: guard
FLT_MAX = 3.4028234663852886e38


@pytest.mark.parametrize("n", [5, 262_149])
def test_adamw_guard(n):
    """pfn_adamw_step_guarded: a guard that is NaN or +-Inf leaves p, m, v and the step number bit-unchanged, counts one skipped
    update and leaves the arrival word 0; any finite guard -- 0, a denormal, a negative number, FLT_MAX -- is the plain update of
    pfn_adamw_step_dev, bit for bit."""
    state = make_state(n, True)
    for gv in (float("nan"), float("inf"), float("-inf")):
        p, m, v, step = launch("guarded", state, T_AXIS, DEFAULTS, guard=gv)
        assert torch.equal(p, state[0]) and torch.equal(m, state[2]) and torch.equal(v, state[3]), gv
        assert step == [T_AXIS, 0, SKIPPED + 1], (gv, step)
    want = launch("dev", state, T_AXIS, DEFAULTS)
    assert not torch.equal(want[0], state[0])
    for gv in (0.0, 1e-40, -3.0, FLT_MAX):
        got = launch("guarded", state, T_AXIS, DEFAULTS, guard=gv)
        assert got[3] == want[3] == [T_AXIS + 1, 0, SKIPPED], (gv, got[3])
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a, b), gv


# ------------------------------------------------------------------------------------------------ AdamW: 300 steps under a schedule
class _ThreeParams(torch.nn.Module):
    """4,099 + 129 + 1 elements, none a multiple of four: the second parameter's view of the flat buffer starts 12 bytes past a
    16-byte boundary, and the flat buffer itself (4,229 floats) ends in a one-element tail."""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(0.1 * torch.randn(4099, generator=gen))
        self.b = torch.nn.Parameter(0.1 * torch.randn(3, 43, generator=gen))
        self.c = torch.nn.Parameter(0.1 * torch.randn(1, generator=gen))


TRAJ_STEPS, TRAJ_MAX_LR, TRAJ_CHECK = 300, 1e-3, (1, 10, 100, 300)
TRAJ_NO_GRAD = (4, 57, 180)      # iterations (0-based) on which parameter `b` has .grad None: FlatAdamW fills zeros


@functools.lru_cache(maxsize=None)
def trajectory_gradients():
    """(300, 4229) fp32: per entry a fixed magnitude (log-uniform over 1e-6 .. 1e1) and drift plus noise, so that signs persist for
    some entries and flip for others.  Open loop: the same sequence feeds every optimizer."""
    gen = torch.Generator().manual_seed(17)
    n = 4099 + 129 + 1
    mag = 10.0 ** (torch.rand(n, generator=gen) * 7.0 - 6.0)
    drift = torch.randn(n, generator=gen)
    return (mag * (drift + torch.randn(TRAJ_STEPS, n, generator=gen))).float().contiguous()


def torch_cpu_trajectory(dtype):
    """torch.optim.AdamW + OneCycleLR on a CPU copy of _ThreeParams in `dtype`: the flat parameters (float64) at the start and after
    the steps of TRAJ_CHECK.  float64 = the reference; float32 = the measurement behind TRAJ_RTOL.  A missing gradient is fed as
    zeros (torch would skip that parameter; FlatAdamW treats it as a zero gradient: decay and moment decay still apply)."""
    model = _ThreeParams().to(dtype)
    params = list(model.parameters())
    opt = torch.optim.AdamW(params, lr=TRAJ_MAX_LR, foreach=False)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=TRAJ_MAX_LR, total_steps=TRAJ_STEPS)
    flat = lambda: torch.cat([p.detach().reshape(-1) for p in params]).double().clone()
    out = {0: flat()}
    grads = trajectory_gradients()
    for k in range(TRAJ_STEPS):
        off = 0
        for p in params:
            g = grads[k, off:off + p.numel()].view(p.shape).to(dtype)
            p.grad = torch.zeros_like(g) if (p is model.b and k in TRAJ_NO_GRAD) else g.clone()
            off += p.numel()
        opt.step()
        sched.step()
        if k + 1 in TRAJ_CHECK:
            out[k + 1] = flat()
    return out


def test_flat_adamw_follows_onecycle_for_300_steps():
    """FlatAdamW under OneCycleLR (lr AND beta1 move every step, through FlatAdamW.hyper) against float64 torch.optim.AdamW under
    the same schedule, same gradients: the state recursion over 300 steps, the device step counter, FlatAdamW._flat_grad's gather
    path with its zero fill.  Then the last 50 steps again with the step captured once in a hipGraph and replayed: bit-identical."""
    from poweflownet_amd.optim import FlatAdamW
    ref = torch_cpu_trajectory(torch.float64)
    grads = trajectory_gradients().to(DEV)
    model = _ThreeParams().to(DEV)
    params = list(model.parameters())
    opt = FlatAdamW(model, lr=TRAJ_MAX_LR)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=TRAJ_MAX_LR, total_steps=TRAJ_STEPS)
    assert opt.flat_param.numel() == 4229 and params[1].data_ptr() % 16 == 12
    static = [torch.zeros_like(p) for p in params]      # the .grad tensors: fixed addresses, so that a captured step reads them

    def feed(k):
        off = 0
        for p, s in zip(params, static):
            s.copy_(grads[k, off:off + p.numel()].view(p.shape))
            p.grad = None if (p is model.b and k in TRAJ_NO_GRAD) else s
            off += p.numel()

    snap = None
    for k in range(TRAJ_STEPS):
        if k == TRAJ_STEPS - 50:
            snap = (opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count.clone(),
                    copy.deepcopy(sched.state_dict()), copy.deepcopy({k_: opt.param_groups[0][k_] for k_ in ("lr", "betas")}))
        feed(k)
        opt.step()
        sched.step()
        if k + 1 in TRAJ_CHECK:
            got = opt.flat_param.double().cpu()
            err, scale = rel_err(got - ref[0], ref[k + 1] - ref[0])
            record(f"parameters after step {k + 1}: displacement vs fp64 torch.optim.AdamW", err, scale, TRAJ_RTOL[k + 1])
            assert err <= TRAJ_RTOL[k + 1] * scale, \
                f"after step {k + 1}: error {err:.3e} = {err / scale:.2e} of the largest displacement {scale:.3e}, bound {TRAJ_RTOL[k + 1]:g}"
            assert torch.equal(params[0].detach().reshape(-1), opt.flat_param[:4099])     # (the parameters ARE the flat buffer)
    assert opt.step_count.tolist() == [TRAJ_STEPS, 0, 0]
    assert opt._gather is not None                                                        # the gather path ran
    eager = (opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())

    # the last 50 again, from the snapshot, as replays of ONE captured step
    for dst, src in zip((opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_count), snap[:4]):
        dst.copy_(src)
    sched.load_state_dict(snap[4])
    opt.param_groups[0].update(snap[5])
    feed(TRAJ_STEPS - 50)
    opt.sync_hyper()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k in range(TRAJ_STEPS - 50, TRAJ_STEPS):
        feed(k)
        opt.sync_hyper()
        graph.replay()
        sched.step()
    torch.cuda.synchronize()
    assert opt.step_count.tolist() == [TRAJ_STEPS, 0, 0]
    for a, b, name in zip((opt.flat_param, opt.exp_avg, opt.exp_avg_sq), eager, ("p", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), f"{name}: 50 replays of the captured step differ from 50 eager steps"


# ------------------------------------------------------------------------------------------------ AdamW: back-to-back launches
def test_adamw_back_to_back_launches_rearm_the_arrival_counter():
    """64 pfn_adamw_step_dev launches on changing gradients with no host synchronisation in between, 256 blocks each: the last
    arriver of every launch bumps the step and re-arms the counter for the next one.  Bit-identical to 64 launches with a
    synchronisation after each, step counter {64, 0, 0}."""
    from poweflownet_amd import _lib as L
    lib = L.load()
    n = 262_149
    p0, _, m0, v0 = make_state(n, True)
    gs = torch.stack([make_state(n, True, seed=s)[1] for s in (1, 2, 3, 4)]).to(DEV)
    hp = torch.tensor(DEFAULTS, dtype=torch.float32, device=DEV)

    def run(sync):
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        step = torch.zeros(3, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        for k in range(64):
            L.check(lib.pfn_adamw_step_dev(p.data_ptr(), gs[k % 4].data_ptr(), m.data_ptr(), v.data_ptr(), n, hp.data_ptr(),
                                           step.data_ptr(), L.stream_ptr()), "pfn_adamw_step_dev")
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return p, m, v, step.tolist()

    a, b = run(False), run(True)
    assert a[3] == [64, 0, 0] and b[3] == [64, 0, 0], (a[3], b[3])
    for x, y, name in zip(a[:3], b[:3], ("p", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), name
    # ... and 64 steps of the float64 recursion (a coarse check that 64 DIFFERENT updates were applied: 1e-5 of the moments)
    p, m, v = p0.double(), m0.double(), v0.double()
    for k in range(64):
        p, m, v = ref_cpu.adamw_step(p, gs[k % 4].cpu(), m, v, k + 1, *widened(DEFAULTS))
    assert_close(a[1].cpu(), m.float(), RTOL, "exp_avg after 64 launches")
    assert_close(a[2].cpu(), v.float(), RTOL, "exp_avg_sq after 64 launches")


# ------------------------------------------------------------------------------------------------ power imbalance
PI_STATS = (torch.tensor([[1.0, -5.0, 25.0, 9.0]]), torch.tensor([[0.04, 12.0, 35.0, 14.0]]),
            torch.tensor([[0.05, 0.2]]), torch.tensor([[0.01, 0.05]]))


def _check_power_imbalance(what, x, edge_index, edge_attr):
    from poweflownet_amd.utils.custom_loss_functions import PowerImbalance
    ea = edge_attr.clamp(-3, 3)                      # r, x stay away from 0 (r = 0.05 + 0.01 ea)
    x_ref = x.double().requires_grad_(True)
    l_ref = ref_cpu.power_imbalance(x_ref, edge_index, ea.double(), *PI_STATS)
    l_ref.backward()
    xd = x.to(DEV).requires_grad_(True)
    loss_fn = PowerImbalance(*PI_STATS)
    for call in range(2):                            # (twice: the arrival counter of the workspace is re-armed)
        xd.grad = None
        loss = loss_fn(xd, edge_index.to(DEV), ea.to(DEV))
        loss.backward(PowerImbalance.unit_grad(loss))
        assert_close(loss, l_ref.float(), RTOL, f"{what}: loss, call {call}")
        assert_close(xd.grad, x_ref.grad.float(), RTOL, f"{what}: grad_x, call {call}")


def test_power_imbalance_above_the_block_cap():
    """71,170 nodes (eleven 6470rte grids): power_imbalance_fwd_kernel's grid is capped at 256 blocks = 65,536 threads, so the first
    5,634 threads take a second node and all 256 partials are combined.  Loss and grad_x against the float64 oracle."""
    from poweflownet_amd.synth import make_batch
    d = make_batch("6470rte", 11, seed=3)
    assert d.x.shape[0] >= 65_536 + 300
    _check_power_imbalance("6470rte x 11", d.x, d.edge_index, d.edge_attr)


def test_power_imbalance_hand_graph():
    """40 nodes: a chain over 0..37, nodes 38 and 39 isolated (no branch: dP, dQ are their own injections), the branch 3-4 stored
    twice (parallel lines) and the pair 10-20 stored in both directions.  The first stored edge has no reverse, so the list counts
    as directed and every stored edge gets a reversed copy -- the pair then appears four times, as it does in the reference."""
    gen = torch.Generator().manual_seed(12)
    chain = torch.stack([torch.arange(0, 37), torch.arange(1, 38)])
    extra = torch.tensor([[3, 10, 20], [4, 20, 10]])
    ei = torch.cat([chain, extra], dim=1)
    assert ref_cpu.is_directed(ei)
    x = torch.randn(40, 4, generator=gen)
    ea = torch.randn(ei.shape[1], 2, generator=gen)
    _check_power_imbalance("hand graph", x, ei, ea)


# ------------------------------------------------------------------------------------------------ MSELoss / Masked_L2_loss
LOSS_COUNTS = [4, 1024, 1028, 261_120, 262_144, 262_148]     # 1 block; 1 -> 2 blocks; 255 blocks -> the 256 cap -> strided


def _loss_inputs(n, seed):
    gen = torch.Generator().manual_seed(100 * seed + n % 89)
    return torch.randn(n, generator=gen) * (1.0 + seed), torch.randn(n, generator=gen)


@pytest.mark.parametrize("n", LOSS_COUNTS)
def test_mse_loss_at_the_block_count_changes(n):
    """pfn_mse_loss, loss and gradient against float64, two calls on different data through one workspace (a counter that is not
    re-armed, or a stale partial, shows in the second); the floats behind the gradient stay untouched."""
    from poweflownet_amd import _lib as L
    lib = L.load()
    ws = torch.zeros(264, device=DEV)
    for call in range(2):
        o, y = _loss_inputs(n, call)
        od, yd = o.to(DEV), y.to(DEV)
        loss = torch.full((1,), SENTINEL, device=DEV)
        grad = torch.full((n + PAD,), SENTINEL, device=DEV)
        L.check(lib.pfn_mse_loss(od.data_ptr(), yd.data_ptr(), n, loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                 L.stream_ptr()), "pfn_mse_loss")
        torch.cuda.synchronize()
        d = o.double() - y.double()
        assert_close(loss[0].cpu(), (d * d).mean().float(), 1e-6, f"n {n}, call {call}: loss")
        assert_close(grad[:n].cpu(), (2.0 * d / n).float(), 1e-6, f"n {n}, call {call}: grad")
        assert bool((grad[n:] == SENTINEL).all().item()), "the floats behind the gradient were written"
        assert int(ws[256:257].view(torch.int32).item()) == 0, "arrival counter not re-armed"


@pytest.mark.parametrize("mask_kind", ["int64", "float"])
@pytest.mark.parametrize("n", LOSS_COUNTS)
def test_masked_l2_loss_at_the_block_count_changes(n, mask_kind):
    """pfn_masked_l2_loss (regularised, regcoeff 0.5; int64 and float masks, the float one with a few 0.5 entries, which belong to
    both index sets) against ref_cpu.masked_l2_loss in float64: loss and gradient, two calls through one workspace."""
    from poweflownet_amd import _lib as L
    from poweflownet_amd.loss import MASKED_L2_WS_FLOATS
    lib = L.load()
    ws = torch.zeros(MASKED_L2_WS_FLOATS, device=DEV)
    for call in range(2):
        o, y = _loss_inputs(n, call)
        gen = torch.Generator().manual_seed(7 + call)
        mask = (torch.rand(n, generator=gen) < 0.4).to(torch.int64)
        mask[call % n] = 1                                   # (neither index set is empty, also at n = 4)
        mask[(call + 1) % n] = 0
        if mask_kind == "float":
            mask = mask.float()
            if n > 4:
                mask[5::97] = 0.5
        o_ref = o.double().requires_grad_(True)
        l_ref = ref_cpu.masked_l2_loss(o_ref, y.double(), mask if mask_kind == "int64" else mask.double(), True, 0.5)
        l_ref.backward()
        od, yd, md = o.to(DEV), y.to(DEV), mask.to(DEV)
        loss = torch.full((1,), SENTINEL, device=DEV)
        grad = torch.full((n + PAD,), SENTINEL, device=DEV)
        L.check(lib.pfn_masked_l2_loss(od.data_ptr(), yd.data_ptr(), md.data_ptr(), 0 if mask_kind == "int64" else 1, n, 1, 0.5,
                                       loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel() * 4, L.stream_ptr()),
                "pfn_masked_l2_loss")
        torch.cuda.synchronize()
        assert_close(loss[0].cpu(), l_ref.detach().float(), 1e-6, f"n {n}, {mask_kind} mask, call {call}: loss")
        assert_close(grad[:n].cpu(), o_ref.grad.float(), 1e-6, f"n {n}, {mask_kind} mask, call {call}: grad")
        assert bool((grad[n:] == SENTINEL).all().item()), "the floats behind the gradient were written"
        assert int(ws[1031:1032].view(torch.int32).item()) == 0, "arrival counter not re-armed"     # MaskedL2Ws::counter, byte 4124
