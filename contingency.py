#!/usr/bin/env python3
"""N-1 line-outage screening of a case: which single line outages overload the rest of the grid?  Every scenario of the test split
of a dataset on disk -- its bus specification and its lines' r and x, read the way dc_error.py reads them -- is screened under the DC
model with line outage distribution factors (`contingency_screen`: two launches for all scenarios and all outages), the worst
outages of every scenario are solved again with the AC solver on the grid without the line (`verify_contingencies`), and the two
are set side by side.  Ratings are `--rating-margin` times the largest base-case flow of a line over the scenarios; a line that
never carries flow is unmonitored.  Without --data-dir the scenarios are `make_physical_inputs`' synthetic ones.  Beyond the dense cap
of the screen (6470rte) the sparse route is taken by itself: one `sparse_plan(mode="dc")` for both screens, three launches each, and
the AC verification on the sparse solver under one cover plan; `--route sparse` asks for it on any case.

    python contingency.py --case 118 --data-dir data [--samples 1000] [--rating-margin 1.5] [--verify-top 5] [--route sparse]

Writes results/<case>_contingency_{severity,worst_line,overloads,islands,base_flow}.npy.

--pairs [--candidates K] goes on to N-2 (`contingency_screen_pairs`) on the route of the N-1 screen -- the sparse route reuses its one
DC plan --: the candidates are the union over the scenarios of each scenario's top-K non-islanding single outages (K defaults to
10), every pair of them is screened with all lines monitored, the worst pairs of every scenario are AC-verified
(`verify_pair_contingencies`, on the sparse solver where the screen took the sparse route), and
results/<case>_contingency_pairs_{severity,worst_line,overloads,islands,pairs}.npy are written too.

--model-run-id R [--cfg_json C] asks the trained NETWORK as well (`contingency_screen_model`): the checkpoint
models/model_R.pt is loaded into the MaskEmbdMultiMPN that C describes (default configs/standard.json), the way error_per_feature.py
loads it; the normalisation statistics are `<data-dir>/params/data_params_R.pt` where that file exists, else those of the training
split of --data-dir (synthetic scenarios have none: identity).  Beside each scenario's top DC outages it prints the network's top
outages with their AC-verified loadings (`verify_contingencies` on the network's result) and writes
results/<case>_contingency_model_{severity,worst_line,overloads}.npy.  Without --model-run-id nothing changes.

--ac [--halves H] adds the AC screen (`contingency_screen_ac`: compensated 1P1Q, H fast-decoupled half-iterations per outage from
the AC base solution, 2 by default) with the same ratings: per scenario its top outages with the DC severity, the 1P1Q severity and
the AC-verified severity side by side, how often each screen names the AC worst line, the voltage figures, and
results/<case>_contingency_ac_{severity,worst_line,overloads,vm_min,vm_min_bus,v_violations,mismatch}.npy.  Where the DC screen takes
the sparse route -- beyond the dense cap by itself, anywhere with --route sparse -- so does the AC screen, under one
`sparse_plan(mode="fd")` built beside the DC plan.

--units [--unit-lines K] [--participation {slack,output}] adds the generator outages (`contingency_screen_units`, the dense routes
only): the units are the PV buses, each losing max(-P, 0) of its scenario; `slack` lets the slack pick the lost output up, `output`
shares it among the other units in proportion to their own output (a = unit_p).  --unit-lines K also screens every unit followed by
a line outage, the lines being the union over the scenarios of each scenario's top-K non-islanding single outages.  It prints every
scenario's top unit outages -- and unit x line items where asked -- DC beside AC-verified (`verify_unit_contingencies`: the bus
types stay, so a PV bus keeps its voltage support) and writes
results/<case>_contingency_units_{units,unit_p,severity,worst_line,overloads}.npy and, with --unit-lines,
results/<case>_contingency_units_{lines,islands,line_severity,line_worst_line,line_overloads}.npy.
"""
import argparse
import os
import sys

import numpy as np


def scenarios(case, data_dir, samples, device, split=(.5, .2, .3)):
    """(bus_type [n], spec [S, n, 4], edge_index [2, e], rx [S, e, 2]) on `device`: the test split of `data_dir`'s case, or synthetic."""
    import torch
    if data_dir is None:
        from poweflownet_amd.synth import CASES, make_physical_inputs
        n, e = CASES[str(case)]
        ei, bt, rx, spec = make_physical_inputs(n, e, samples or 64, seed=0)
        return bt.to(device), spec.to(device), ei.to(device), rx.to(device)
    from dc_error import load_test_split, solver_inputs
    _, node, edge = load_test_split(data_dir, case, samples, split)
    if (edge[:, :, :2] != edge[:1, :, :2]).any():
        raise RuntimeError("contingency: the scenarios have different line lists; the screen takes one list for all")
    spec, ei, rx = solver_inputs(node, edge, device)
    return torch.from_numpy(node[0, :, 1].astype(np.int64)).to(device), spec, ei[0].contiguous(), rx


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", default="118")
    ap.add_argument("--data-dir", default=None, help="dataset root; without it: synthetic scenarios of the case's size")
    ap.add_argument("--samples", type=int, default=None, help="only the first N scenarios of the test split (synthetic: 64)")
    ap.add_argument("--rating-margin", type=float, default=1.5, help="rating = margin x the line's largest base-case flow")
    ap.add_argument("--verify-top", type=int, default=5, help="AC-verify the worst N non-islanding outages of every scenario")
    ap.add_argument("--route", default="auto", choices=("auto", "lds", "global", "sparse"),
                    help="auto: the dense screen up to its cap, the sparse route beyond")
    ap.add_argument("--pairs", action="store_true", help="also screen the pairs of the worst single outages (N-2) on the same route")
    ap.add_argument("--candidates", type=int, default=10, help="--pairs: every scenario's top K non-islanding outages are candidates")
    ap.add_argument("--split", type=float, nargs=3, default=[.5, .2, .3], help="train / val / test fractions of the dataset")
    ap.add_argument("--out-dir", default="results")
    ap.add_argument("--model-run-id", default=None, help="also screen with the network of models/model_<id>.pt (contingency_screen_model)")
    ap.add_argument("--cfg_json", default="configs/standard.json", help="--model-run-id: the network's hidden_dim, n_gnn_layers, K")
    ap.add_argument("--ac", action="store_true", help="also screen under AC by compensated 1P1Q (contingency_screen_ac) on the route of the DC screen")
    ap.add_argument("--halves", type=int, default=2, help="--ac: fast-decoupled half-iterations per outage (2: 1P1Q, 4: 2P2Q)")
    ap.add_argument("--units", action="store_true", help="also screen the outage of every unit (the PV buses) under DC (contingency_screen_units)")
    ap.add_argument("--unit-lines", type=int, default=0, help="--units: every unit followed by each of every scenario's top K non-islanding line outages")
    ap.add_argument("--participation", default="slack", choices=("slack", "output"),
                    help="--units: who picks the lost output up -- the slack, or the other units in proportion to their output")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("contingency.py needs a HIP device: poweflownet_amd has no CPU solver")
    from poweflownet_amd.utils.contingency import contingency_screen, verify_contingencies
    from poweflownet_amd.utils.powerflow import max_unknowns, sparse_plan
    bt, spec, ei, rx = scenarios(a.case, a.data_dir, a.samples, "cuda:0", tuple(a.split))
    S, e = int(spec.shape[0]), int(ei.shape[1])
    kw, solver_kw = {"route": a.route}, {}
    if a.route == "sparse" or (a.route == "auto" and int(bt.shape[0]) - 1 > max_unknowns()):
        plan = sparse_plan(bt, ei, mode="dc")                              # once: both screens share it
        print(f"sparse route: {plan.m} unknowns, nnz(L) {plan.nnz_l}, plan built in {plan.build_s:.2f} s")
        kw, solver_kw = {"route": "sparse", "plan": plan}, {"route": "sparse"}
    base = contingency_screen(bt, spec, ei, rx, **kw)                       # the base flows decide the ratings
    if int((base.status < 0).sum()):
        raise RuntimeError(f"contingency: {int((base.status < 0).sum())} base cases failed (statuses {sorted(set(base.status.tolist()))})")
    ratings = a.rating_margin * base.base_flow.abs().max(dim=0).values     # [e]; 0 where a line never carries flow: unmonitored
    res = contingency_screen(bt, spec, ei, rx, ratings, **kw)
    islands = res.islands.cpu().numpy()
    print(f"Case {a.case}: {S} scenarios x {e} outages on the {res.route} route; {int((ratings > 0).sum())} of {e} lines monitored")
    print(f"{int((islands > 0).sum())} islanding outages, {int(islands[islands > 0].sum())} buses lost over them")
    top = min(a.verify_top, int((islands == 0).sum()))
    ver = verify_contingencies(res, bt, spec, ei, rx, ratings, top=top, **solver_kw)
    pairs, dc, ac = ver.pairs.cpu().numpy(), ver.dc_severity.cpu().numpy(), ver.severity.cpu().numpy()
    dc_worst, ac_worst = res.worst_line[ver.pairs[:, 0], ver.pairs[:, 1]].cpu().numpy(), ver.worst_line.cpu().numpy()
    status = ver.status.cpu().numpy()
    for s in range(S):
        rows = [f"line {pairs[t, 1]}: DC {dc[t]:.3f} AC {'failed' if status[t] < 0 else format(ac[t], '.3f')} "
                f"worst line {dc_worst[t]}{'=' if dc_worst[t] == ac_worst[t] else '!='}{ac_worst[t]}" for t in np.flatnonzero(pairs[:, 0] == s)]
        print(f"scenario {s}: " + "; ".join(rows))
    solved = status >= 0
    missed = int((solved & (dc < 1) & (ac > 1)).sum())
    agree = int((solved & (dc_worst == ac_worst)).sum())
    print(f"{len(pairs)} pairs verified, {int((~solved).sum())} AC solves failed; worst line agrees in {agree}; "
          f"{missed} of {int((solved & (dc < 1)).sum())} the DC screen called secure are overloaded under AC")
    os.makedirs(a.out_dir, exist_ok=True)
    for name in ("severity", "worst_line", "overloads", "islands", "base_flow"):
        np.save(os.path.join(a.out_dir, f"case{a.case}_contingency_{name}.npy"), getattr(res, name).cpu().numpy())
    if a.pairs:
        screen_pairs(a, res, islands, bt, spec, ei, rx, ratings, kw, solver_kw)
    if a.model_run_id is not None:
        screen_model(a, islands, bt, spec, ei, rx, ratings, solver_kw)
    if a.ac:
        screen_ac(a, res, islands, bt, spec, ei, rx, ratings, solver_kw, sparse=kw["route"] == "sparse")
    if a.units:
        screen_units(a, res, islands, bt, spec, ei, rx, ratings, kw)
    return 0


def screen_units(a, res, islands, bt, spec, ei, rx, ratings, kw):
    """--units: the generator outages of the same scenarios with the same ratings on the N-1 screen's dense route, with --unit-lines
    followed by the worst single line outages; DC beside AC-verified, and the result files"""
    from poweflownet_amd.utils.contingency import contingency_screen_units, verify_unit_contingencies
    if kw["route"] == "sparse":
        raise SystemExit("contingency.py --units: the sparse route of the unit screen is not built; this case is beyond the dense cap")
    if a.unit_lines < 0:
        raise SystemExit("contingency.py --units: --unit-lines must be >= 0")
    S, e = int(spec.shape[0]), int(ei.shape[1])
    lines = None
    if a.unit_lines:
        order = res.ranking(e)[0].cpu().numpy()
        lines = sorted({int(k) for s in range(S) for k in [k for k in order[s] if islands[k] == 0][:a.unit_lines]}) or None
    first = contingency_screen_units(bt, spec, ei, rx, ratings, route=kw["route"])      # (units=None: the PV buses; unit_p=None: max(-P, 0))
    part = first.unit_p.contiguous() if a.participation == "output" else None
    got = first if part is None and lines is None else contingency_screen_units(bt, spec, ei, rx, ratings, participation=part, lines=lines,
                                                                                   route=kw["route"])
    units = got.units.cpu().numpy()
    G = len(units)
    print(f"units: {G} PV buses x {S} scenarios on the {got.route} route, lost output picked up by "
          f"{'the slack' if part is None else 'the other units in proportion to their output'}"
          + (f"; {len(lines)} lines (top {a.unit_lines} of every scenario) behind every unit" if lines else ""))
    ver = verify_unit_contingencies(got, bt, spec, ei, rx, ratings, top=min(a.verify_top, G))
    items, dc, ac, status = ver.items.cpu().numpy(), ver.dc_severity.cpu().numpy(), ver.severity.cpu().numpy(), ver.status.cpu().numpy()
    ac_worst = ver.worst_line.cpu().numpy()
    for s in range(S):
        for lined, label in ((False, "units"), (True, "unit x line")):
            rows = [f"bus {units[items[t, 1]]}" + (f"+line {items[t, 2]}" if lined else "") + f": DC {dc[t]:.3f} "
                    f"AC {'failed' if status[t] < 0 else format(ac[t], '.3f')} worst line {ac_worst[t]}"
                    for t in np.flatnonzero((items[:, 0] == s) & ((items[:, 2] >= 0) == lined))]
            if rows:
                print(f"scenario {s} {label}: " + "; ".join(rows))
    solved = status >= 0
    print(f"{len(items)} unit items verified, {int((~solved).sum())} AC solves failed; "
          f"{int((solved & (dc < 1) & (ac > 1)).sum())} of {int((solved & (dc < 1)).sum())} the DC unit screen called secure are overloaded under AC")
    names = ["units", "unit_p", "severity", "worst_line", "overloads"] + (["lines", "islands", "line_severity", "line_worst_line", "line_overloads"] if lines else [])
    for name in names:
        np.save(os.path.join(a.out_dir, f"case{a.case}_contingency_units_{name}.npy"), getattr(got, name).cpu().numpy())


def screen_ac(a, dc_res, islands, bt, spec, ei, rx, ratings, solver_kw, sparse=False):
    """--ac: the AC screen of the same scenarios with the same ratings on the DC screen's route (`sparse`: under one fast-decoupled
    plan built here), its worst outages AC-verified beside the DC screen's figures, the voltage figures, and the seven result files"""
    import torch

    from poweflownet_amd.utils.contingency import contingency_screen_ac, verify_contingencies
    from poweflownet_amd.utils.powerflow import sparse_plan
    kw = {}
    if sparse:
        plan = sparse_plan(bt, ei, mode="fd")                              # once, beside the DC plan
        print(f"sparse route of the AC screen: B' of {plan.m} and B'' of {plan.m_q} unknowns, nnz(L) {plan.nnz_l}, plan built in {plan.build_s:.2f} s")
        kw = {"route": "sparse", "plan": plan}
    res = contingency_screen_ac(bt, spec, ei, rx, ratings, halves=a.halves, **kw)
    S, e = int(spec.shape[0]), int(ei.shape[1])
    failed = int((res.status < 0).sum())
    where = (f"sparse factors, 64 outages per workgroup, blocks on the {res.block} placement" if sparse
             else f"inverses on the {res.route} placement, {res.group} outages per workgroup")
    print(f"AC screen: {a.halves} half-iterations per outage, {S} scenarios x {e} outages, {where}; "
          f"base solves {int(res.status.clamp(min=0).max())} half-iterations at most, {failed} failed")
    top = min(a.verify_top, int((islands == 0).sum()))
    ver = verify_contingencies(res, bt, spec, ei, rx, ratings, top=top, **solver_kw)
    sc, out = ver.pairs[:, 0], ver.pairs[:, 1]
    pairs, fd, ac, status = ver.pairs.cpu().numpy(), ver.dc_severity.cpu().numpy(), ver.severity.cpu().numpy(), ver.status.cpu().numpy()
    dc = dc_res.severity[sc, out].cpu().numpy()                            # (dc_severity above: this screen's figure, the 1P1Q one)
    dc_worst, fd_worst, ac_worst = dc_res.worst_line[sc, out].cpu().numpy(), res.worst_line[sc, out].cpu().numpy(), ver.worst_line.cpu().numpy()
    vmin, vbus, vviol = (getattr(res, k)[sc, out].cpu().numpy() for k in ("vm_min", "vm_min_bus", "v_violations"))
    mis = res.mismatch[sc, out].cpu().numpy()
    for s in range(S):
        rows = [f"line {pairs[t, 1]}: DC {dc[t]:.3f} 1P1Q {fd[t]:.3f} AC {'failed' if status[t] < 0 else format(ac[t], '.3f')} "
                f"worst line {dc_worst[t]}/{fd_worst[t]}/{ac_worst[t]} Vmin {vmin[t]:.3f} at bus {vbus[t]} ({vviol[t]} outside) mismatch {mis[t]:.1e}"
                for t in np.flatnonzero(pairs[:, 0] == s)]
        print(f"scenario {s} AC screen: " + "; ".join(rows))
    solved = status >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        err_dc, err_fd = (np.abs(v - ac)[solved & np.isfinite(v)] / ac[solved & np.isfinite(v)] for v in (dc, fd))
    med = lambda v: float(np.median(v)) if v.size else float("nan")           # noqa: E731
    print(f"{len(pairs)} pairs verified, {int((~solved).sum())} AC solves failed; worst line equals AC's: DC {int((solved & (dc_worst == ac_worst)).sum())}, "
          f"1P1Q {int((solved & (fd_worst == ac_worst)).sum())}; relative severity error, median: DC {med(err_dc):.2g}, 1P1Q {med(err_fd):.2g}; "
          f"{int((solved & (fd < 1) & (ac > 1)).sum())} of {int((solved & (fd < 1)).sum())} the AC screen called secure are overloaded under AC")
    ok = (res.islands == 0)[None, :] & (res.status >= 0)[:, None]
    low = torch.where(ok, res.vm_min, torch.full_like(res.vm_min, float("inf")))
    print(f"voltage: lowest Vm over all screened outages {float(low.min()):.4f}; {int((ok & (res.v_violations > 0)).sum())} of {int(ok.sum())} "
          f"(scenario, outage) pairs leave a PQ bus outside the limits; largest mismatch {float(res.mismatch[ok].max()) if bool(ok.any()) else float('nan'):.2e}")
    for name in ("severity", "worst_line", "overloads", "vm_min", "vm_min_bus", "v_violations", "mismatch"):
        np.save(os.path.join(a.out_dir, f"case{a.case}_contingency_ac_{name}.npy"), getattr(res, name).cpu().numpy())


def model_statistics(a):
    """{xymean, xystd, edgemean, edgestd} of the run: its saved parameters, else the training split's own; synthetic: none"""
    import torch
    if a.data_dir is None:
        print("synthetic scenarios carry no statistics: the network sees them un-normalised")
        return {}
    names = ("xymean", "xystd", "edgemean", "edgestd")
    params = os.path.join(a.data_dir, "params", f"data_params_{a.model_run_id}.pt")
    if os.path.exists(params):
        p = torch.load(params, map_location="cpu")
        return {k: p[k] for k in names}
    from poweflownet_amd.datasets import PowerFlowData
    print(f"no {params}: the statistics of the training split are taken")
    train = PowerFlowData(root=a.data_dir, case=a.case, split=list(a.split), task="train")
    return dict(zip(names, train.get_data_means_stds()))


def screen_model(a, islands, bt, spec, ei, rx, ratings, solver_kw):
    """--model-run-id: the network's screen of the same scenarios, its worst outages AC-verified, and the three result files"""
    import json

    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.utils.contingency import contingency_screen_model, verify_contingencies
    from poweflownet_amd.utils.evaluation import load_model
    cfg_path = a.cfg_json if os.path.exists(a.cfg_json) else os.path.join(os.path.dirname(os.path.abspath(__file__)), a.cfg_json)
    with open(cfg_path) as f:
        cfg = json.load(f)
    model = MaskEmbdMultiMPN(nfeature_dim=4, efeature_dim=2, output_dim=4, hidden_dim=int(cfg["hidden_dim"]), n_gnn_layers=int(cfg["n_gnn_layers"]),
                             K=int(cfg["K"]), dropout_rate=float(cfg["dropout_rate"])).to(spec.device)
    model, _ = load_model(model, a.model_run_id, spec.device)
    res = contingency_screen_model(model, bt, spec, ei, rx, ratings, **model_statistics(a))
    S, e = int(spec.shape[0]), int(ei.shape[1])
    print(f"network {a.model_run_id}: {S} scenarios x {e} outages in chunks of {res.chunk} items")
    top = min(a.verify_top, int((islands == 0).sum()))
    ver = verify_contingencies(res, bt, spec, ei, rx, ratings, top=top, **solver_kw)
    pairs, net, ac = ver.pairs.cpu().numpy(), ver.dc_severity.cpu().numpy(), ver.severity.cpu().numpy()    # (dc_severity: the network's figure)
    net_worst, ac_worst = res.worst_line[ver.pairs[:, 0], ver.pairs[:, 1]].cpu().numpy(), ver.worst_line.cpu().numpy()
    status = ver.status.cpu().numpy()
    for s in range(S):
        rows = [f"line {pairs[t, 1]}: network {net[t]:.3f} AC {'failed' if status[t] < 0 else format(ac[t], '.3f')} "
                f"worst line {net_worst[t]}{'=' if net_worst[t] == ac_worst[t] else '!='}{ac_worst[t]}" for t in np.flatnonzero(pairs[:, 0] == s)]
        print(f"scenario {s} network: " + "; ".join(rows))
    solved = status >= 0
    with np.errstate(invalid="ignore"):
        gap = np.abs(net - ac)[solved & np.isfinite(net)]
    print(f"{len(pairs)} pairs verified, {int((~solved).sum())} AC solves failed; worst line agrees in {int((solved & (net_worst == ac_worst)).sum())}; "
          f"|network - AC| severity: mean {gap.mean() if gap.size else float('nan'):.3g}, max {gap.max() if gap.size else float('nan'):.3g}; "
          f"{int((solved & (net < 1) & (ac > 1)).sum())} of {int((solved & (net < 1)).sum())} the network called secure are overloaded under AC")
    for name in ("severity", "worst_line", "overloads"):
        np.save(os.path.join(a.out_dir, f"case{a.case}_contingency_model_{name}.npy"), getattr(res, name).cpu().numpy())


def screen_pairs(a, res, islands, bt, spec, ei, rx, ratings, kw, solver_kw):
    """--pairs: N-2 among the worst single outages on the N-1 screen's route (`kw`: its route and plan), DC beside AC (`solver_kw`:
    the AC solver's route), and the five result files"""
    from poweflownet_amd.utils.contingency import contingency_screen_pairs, verify_pair_contingencies
    if a.candidates < 2:
        raise SystemExit("contingency.py --pairs: --candidates must be at least 2")
    S, e = int(spec.shape[0]), int(ei.shape[1])
    order = res.ranking(e)[0].cpu().numpy()
    lines = sorted({int(k) for s in range(S) for k in [k for k in order[s] if islands[k] == 0][:a.candidates]})
    if len(lines) < 2:
        raise SystemExit(f"contingency.py --pairs: {len(lines)} non-islanding outage(s) leave no pair to screen")
    two = contingency_screen_pairs(bt, spec, ei, rx, ratings, lines=lines, **kw)
    pair_islands = two.islands.cpu().numpy()
    held = two.pairs.cpu().numpy()
    print(f"N-2: {len(lines)} candidate lines (top {a.candidates} of every scenario), {len(held)} pairs x {S} scenarios on the {two.route} route")
    print(f"{int((pair_islands > 0).sum())} islanding pairs of non-islanding outages, {int(pair_islands[pair_islands > 0].sum())} buses lost over them")
    top = min(a.verify_top, int((pair_islands == 0).sum()))
    ver = verify_pair_contingencies(two, bt, spec, ei, rx, ratings, top=top, **solver_kw)
    triples, dc, ac, status = ver.triples.cpu().numpy(), ver.dc_severity.cpu().numpy(), ver.severity.cpu().numpy(), ver.status.cpu().numpy()
    dc_worst, ac_worst = two.worst_line[ver.triples[:, 0], ver.pair_index].cpu().numpy(), ver.worst_line.cpu().numpy()
    for s in range(S):
        rows = [f"lines {triples[t, 1]}+{triples[t, 2]}: DC {dc[t]:.3f} AC {'failed' if status[t] < 0 else format(ac[t], '.3f')} "
                f"worst line {dc_worst[t]}{'=' if dc_worst[t] == ac_worst[t] else '!='}{ac_worst[t]}" for t in np.flatnonzero(triples[:, 0] == s)]
        print(f"scenario {s} pairs: " + "; ".join(rows))
    solved = status >= 0
    print(f"{len(triples)} (scenario, pair) rows verified, {int((~solved).sum())} AC solves failed; worst line agrees in "
          f"{int((solved & (dc_worst == ac_worst)).sum())}; {int((solved & (dc < 1) & (ac > 1)).sum())} of {int((solved & (dc < 1)).sum())} "
          f"the DC pair screen called secure are overloaded under AC")
    for name in ("severity", "worst_line", "overloads", "islands", "pairs"):
        np.save(os.path.join(a.out_dir, f"case{a.case}_contingency_pairs_{name}.npy"), getattr(two, name).cpu().numpy())


if __name__ == "__main__":
    sys.exit(main())
