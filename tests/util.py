"""Shared helpers for the parity tests (fixture loading, tolerances, the float64 oracle on the HIP path's own ReLU decisions)."""
import copy
import os

import numpy as np
import torch

from poweflownet_amd.data import Data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# north_star tolerance: 1e-5 relative, fp32.  "Relative" is normwise and FLAT: |a - b| <= RTOL * max|b| for every element
# (no extra elementwise slack).  Every comparison also records the error it achieved (`REPORT`), which conftest.py dumps
# to gpurun_out/parity_report.json at the end of a GPU session -- the bounds in the tests are set from those numbers.
RTOL = 1e-5
REPORT = {}


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiub" and z[k].dtype != np.bool_ else z[k]
            for k in z.files}


def data_from(fx, prefix="", device=None):
    d = Data(**{k: fx[prefix + k] for k in ("x", "y", "bus_type", "pred_mask", "edge_index", "edge_attr")})
    if prefix + "batch" in fx:
        d.batch = fx[prefix + "batch"]
    else:
        d.batch = torch.zeros(d.x.shape[0], dtype=torch.long)
    return d.to(device) if device is not None else d


def params_from(fx, prefix="param."):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def rel_err(a, b):
    """(max |a - b|, max |b|) in float64."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    if b.numel() == 0:
        return 0.0, 0.0
    return (a - b).abs().max().item(), b.abs().max().item()


def record(what, err, scale, bound=None):
    import os
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    REPORT.setdefault(test, []).append({"what": what, "max_abs_err": err, "scale": scale,
                                        "rel": (err / scale if scale > 0 else 0.0), "bound_rel": bound})


def assert_close(a, b, rtol=RTOL, what=""):
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if b.numel() == 0:
        return
    err, scale = rel_err(a, b)
    record(what, err, scale, rtol)
    assert err <= rtol * scale + 1e-30, \
        f"{what}: max err {err:.3e} = {err / max(scale, 1e-300):.2e} of the largest entry {scale:.3e}, bound {rtol:g}"


def record_elementwise(a, b, what, rtol=1e-5, atol_of_max=1e-6):
    """The ELEMENTWISE reading of "1e-5 relative" next to the normwise one of assert_close: how many entries violate
    |a - b| <= rtol * |b| + atol_of_max * max|b|, and by how much at worst.  Recorded (gpurun_out/parity_report.json), returned as
    (violations, entries, worst ratio err / bound)."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    if b.numel() == 0:
        return 0, 0, 0.0
    bound = rtol * b.abs() + atol_of_max * b.abs().max()
    ratio = ((a - b).abs() / bound.clamp_min(1e-300))
    bad, worst = int((ratio > 1.0).sum()), float(ratio.max())
    record(f"{what}: elementwise |a-b| <= {rtol:g}|b| + {atol_of_max:g} max|b|: {bad} of {b.numel()} entries exceed it, worst {worst:.3f} x the bound",
           float((a - b).abs().max()), float(b.abs().max()), None)
    return bad, b.numel(), worst


# ------------------------------------------------------------------ oracle comparisons shared by the GPU test modules
DEV = "cuda:0"


def _exported_masks(m, n_rows):
    """Keep masks (N, H) of the hidden layers for the model's CURRENT dropout state (= the last training forward)."""
    from poweflownet_amd import _lib as L
    masks = []
    for li in range(len(m.layers) - 1):
        k = torch.empty(n_rows, m.hidden_dim, device=DEV)
        L.check(L.load().pfn_dropout_mask(m._rng_state.data_ptr(), li, n_rows, m.hidden_dim, float(m.dropout_rate),
                                          k.data_ptr(), L.stream_ptr()), "pfn_dropout_mask")
        masks.append(k)
    return masks


def _to64(data):
    d64 = data.clone()
    d64.x, d64.y, d64.edge_attr = data.x.double(), data.y.double(), data.edge_attr.double()
    d64.pred_mask = data.pred_mask.double()
    return d64


def _fp64_truth(ref32, data):
    """The same oracle in float64, on its OWN ReLU decisions (forward yardstick)."""
    ref64 = copy.deepcopy(ref32).double()
    ref64.recorded_gates = {}
    with torch.no_grad():
        out = ref64(_to64(data))
    return out, ref64.recorded_gates


def _gate_differences(a, b):
    """Number of ReLU decisions that differ between two gate sets, per site."""
    diff = {"mask_embd": int((a["mask_embd"] != b["mask_embd"]).sum())}
    for kind in ("edge", "out"):
        for li in a[kind]:
            diff[f"{kind}.{li}"] = int((a[kind][li] != b[kind][li]).sum())
    return diff


def _cpu_gates(m):
    g = m.export_gates()                      # (the workspace lives as long as the forward's output / loss do)
    return {"mask_embd": g["mask_embd"].cpu(), "edge": {k: v.cpu() for k, v in g["edge"].items()},
            "out": {k: v.cpu() for k, v in g["out"].items()}}


def _assert_grads_on_hip_gates(m, ref, data, what, out=None, gates=None):
    """Call right after `m`'s backward.  A network with ~10^7 ReLU units has a few pre-activations within the fp32 forward error
    of zero, whose gate differs between ANY two arithmetic orders (one flipped gate moves a weight gradient by 1e-5..2e-4 of its
    largest entry -- a property of the function, not of the kernels).  So the float64 oracle is run on the gate decisions the HIP
    forward actually took (`export_gates`, `ref_cpu.gated_relu`) -- the same piecewise-linear branch -- and then EVERY parameter
    gradient must match at north_star's 1e-5 of its largest entry."""
    ref64 = copy.deepcopy(ref).double()       # (a train-mode oracle carries its dropout_masks along)
    ref64.zero_grad(set_to_none=True)         # (... and any gradients `ref` already holds, which must not accumulate)
    ref64.gates = gates if gates is not None else _cpu_gates(m)
    d64 = _to64(data)
    o64 = ref64(d64)
    if out is not None:
        assert_close(out, o64.float(), RTOL, f"{what}: out vs fp64 oracle on the HIP gates")
    torch.nn.MSELoss()(o64, d64.y).backward()
    for (k, p), t in zip(m.named_parameters(), ref64.parameters()):
        assert_close(p.grad, t.grad, RTOL, f"{what}: grad.{k} vs fp64 oracle on the HIP gates")


def _check_full_size(m, ref, data, what, max_flips_per_site=64, ungated=False):
    """Forward + every parameter gradient of the HIP model `m` (eval mode, parameters == `ref`'s) at a BASELINE.json size.
    Forward: north_star's 1e-5 against the fp32 oracle AND the float64 oracle (each on its own ReLU decisions).  Gradients:
    1e-5 against the float64 oracle held to the HIP forward's ReLU decisions (_assert_grads_on_hip_gates); the number of
    decisions that differ from float64's own is counted per site and must be tiny."""
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    with torch.no_grad():
        out_ref = ref(data)
    out64, own64 = _fp64_truth(ref, data)
    dd = data.to(DEV)
    m.zero_grad(set_to_none=True)
    out = m(dd)
    assert_close(out, out_ref, RTOL, f"{what}: out vs fp32 oracle")
    assert_close(out, out64.float(), RTOL, f"{what}: out vs fp64 oracle")
    # ... and the elementwise reading of the same tolerance (entries far below the tensor's maximum get a relative bound too):
    # |a - b| <= 1e-5 |b| + 1e-6 max|b|.  RECORDED for both the HIP path and the fp32 oracle (gpurun_out/parity_report.json; round 5:
    # 0 entries exceed it at configs 3 and 4, 1 of 60,416 at config 2 at 1.2 x the bound, 17 of 60,416 for hidden 512 at 2.0 x --
    # the MFMA k order against the oracle's); asserted only as far as that justifies: <= 0.1 % of the entries, none beyond 4 x.
    bad, total, worst = record_elementwise(out, out64, f"{what}: out vs fp64 oracle")
    record_elementwise(out_ref, out64, f"{what}: fp32 ORACLE out vs fp64 oracle")
    assert bad <= 1e-3 * total and worst <= 4.0, (what, bad, total, worst)
    loss = torch.nn.MSELoss()(out, dd.y)
    loss.backward()
    gates = _cpu_gates(m)
    flips = _gate_differences(gates, own64)
    total = sum(g.numel() for g in [gates["mask_embd"], *gates["edge"].values(), *gates["out"].values()])
    record(f"{what}: ReLU decisions differing from float64's own: {sum(flips.values())} of {total} {flips}", 0.0, 1.0, None)
    assert max(flips.values()) <= max_flips_per_site, flips
    del own64
    _assert_grads_on_hip_gates(m, ref, data, what, out, gates)
    if ungated:
        # the UNMODIFIED reference dataflow: the fp32 oracle on its own ReLU decisions.  A handful of flipped gates moves single
        # weight gradients by 1e-5..2e-4 of their largest entry (see _assert_grads_on_hip_gates), so this is RECORDED, and
        # bounded only by what two fp32 arithmetic orders of the same function can differ by
        ref.zero_grad(set_to_none=True)
        torch.nn.MSELoss()(ref(data), data.y).backward()
        worst = 0.0
        for (k, p), t in zip(m.named_parameters(), ref.parameters()):
            err, scale = rel_err(p.grad, t.grad)
            record(f"{what}: grad.{k} vs the UNGATED fp32 oracle", err, scale, 5e-4)
            worst = max(worst, err / max(scale, 1e-300))
        ref.zero_grad(set_to_none=True)
        assert worst <= 5e-4, (what, worst)


# ------------------------------------------------------------------ one profiled training step with or without an attached loss
def _run(m, d, loss_fn, attach, x_grad=False):
    from poweflownet_amd import _lib as L
    m.seed_dropout(78)
    m.zero_grad(set_to_none=True)
    d.x.grad = None
    d.x.requires_grad_(x_grad)
    L.profile_report(reset=True)
    L.profile_enable(True)
    if attach:
        loss_fn.attach(m, d.y)
    out = m(d)
    loss = loss_fn(out, d.y)
    loss.backward(loss_fn.unit_grad(loss))
    torch.cuda.synchronize()
    L.profile_enable(False)
    rep = L.profile_report(reset=True)
    launches = {k: v["count"] for k, v in rep.items() if not k.startswith("__")}
    return {"out": out.detach().clone(), "loss": loss.detach().clone(), "g": m.flat_grad().clone(),
            "gx": d.x.grad.clone() if x_grad else None, "launches": launches}


def _run_masked(m, d, loss_fn, attach):
    from poweflownet_amd import _lib as L
    m.seed_dropout(78)
    m.zero_grad(set_to_none=True)
    L.profile_report(reset=True)
    L.profile_enable(True)
    if attach:
        loss_fn.attach(m, d.y, d.pred_mask)
    out = m(d)
    loss = loss_fn(out, d.y, d.pred_mask)
    loss.backward(loss_fn.unit_grad(loss))
    torch.cuda.synchronize()
    L.profile_enable(False)
    rep = L.profile_report(reset=True)
    return {"out": out.detach().clone(), "loss": loss.detach().clone(), "g": m.flat_grad().clone(),
            "launches": {k: v["count"] for k, v in rep.items() if not k.startswith("__")}}
