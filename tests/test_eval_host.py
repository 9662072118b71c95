"""Host side of the evaluation report: `report_from_accumulators` against the float64 formulas on synthetic accumulators, its key
list against the lines test.py prints, and the term table of `_lib` against the enumerators of include/pfn_hip.h.  No GPU."""
import os
import re

import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.utils.custom_loss_functions import MaskedL1, MaskedL2V2
from poweflownet_amd.utils.evaluation import _RunningSum, report_from_accumulators, report_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = torch.tensor([0.05, 10.0, 50.0, 20.0], dtype=torch.float64)
MEAN = torch.tensor([1.0, 0.0, 30.0, 10.0], dtype=torch.float64)


def _batch_terms(o, y, m):
    """The batch terms of pfn_eval_metrics in float64, in L.EVAL_TERMS order."""
    t = {f"cnt_{n}": float(m[:, f].sum()) for f, n in enumerate(("vm", "va", "p", "q"))}
    for fam, loss, a, b in (("l2", MaskedL2V2(), o, y), ("l1", MaskedL1(), o, y),
                            ("l2d", MaskedL2V2(), o * STD + MEAN, y * STD + MEAN), ("l1d", MaskedL1(), o * STD + MEAN, y * STD + MEAN)):
        for k, v in loss(a, b, m).items():
            t[f"{fam}_{'balanced' if k == 'balanced total' else k}"] = float(v)
    d2 = (o - y) ** 2
    t["ml2_selected"] = float(d2[m != 0].mean())
    t["ml2_regularizer"] = float(d2[(1 - m) != 0].mean())
    t["mse"] = float(d2.mean())
    return [t[name] for name in L.EVAL_TERMS]


@pytest.mark.parametrize("first_unweighted", [True, False])
def test_report_from_accumulators_against_the_float64_formulas(first_unweighted):
    g = torch.Generator().manual_seed(3)
    sizes, n_keys = (112, 112, 84), 8
    batches = []
    for n in sizes:
        o = torch.randn(n, 4, generator=g, dtype=torch.float64)
        batches.append((o, o + 0.1 * torch.randn(n, 4, generator=g, dtype=torch.float64), torch.randint(0, 2, (n, 4), generator=g)))
    acc, pi, num = [0.0] * len(L.EVAL_TERMS), [0.0, 0.0], 0
    for b, (o, y, m) in enumerate(batches):
        w = 1.0 if (first_unweighted and b == 0) else float(n_keys)
        for k, v in enumerate(_batch_terms(o, y, m)):
            acc[k] += v * w
        pi[0] += (0.5 + b) * w
        pi[1] += (0.25 + b) * w
        num += n_keys
    rep = report_from_accumulators(acc, num, tuple(pi))
    # the same report the way evaluate_epoch_v2 forms it: per loss, per term, with its weighting
    want = {}
    for title, loss, de in (("MaskedL2", MaskedL2V2(), False), ("MaskedL2(denorm)", MaskedL2V2(), True), ("MaskedL1(denorm)", MaskedL1(), True)):
        tot = None
        for b, (o, y, m) in enumerate(batches):
            terms = loss(o * STD + MEAN, y * STD + MEAN, m) if de else loss(o, y, m)
            w = 1.0 if (first_unweighted and b == 0) else float(n_keys)
            tot = {k: (0.0 if tot is None else tot[k]) + float(v) * w for k, v in terms.items()}
        for k, v in tot.items():
            want[f"{title} {k}"] = v / num
    for b, (o, y, m) in enumerate(batches):
        w = 1.0 if (first_unweighted and b == 0) else float(n_keys)
        d2 = (o - y) ** 2
        want["PowerImbalance"] = want.get("PowerImbalance", 0.0) + (0.5 + b) * w / num
        want["PowerImbalance(ref)"] = want.get("PowerImbalance(ref)", 0.0) + (0.25 + b) * w / num
        want["Masked_L2_loss"] = want.get("Masked_L2_loss", 0.0) + float(d2[m != 0].mean()) * w / num
        want["MSE"] = want.get("MSE", 0.0) + float(d2.mean()) * w / num
    assert list(rep) == list(want) == report_keys()
    for k in want:
        assert rep[k] == pytest.approx(want[k], rel=1e-12), k
    assert list(report_from_accumulators(acc, num)) == report_keys(power_imbalance=False)
    with pytest.raises(ValueError):
        report_from_accumulators(acc[:5], num)


def test_report_keys_are_the_lines_test_py_prints():
    """test.py's six-pass loop prints f"{title} {key}:" per MaskedL2V2 / MaskedL1 term and f"{name}:" (+ "(ref)") for the rest:
    the titles and names are read from its source, the term keys from the losses themselves."""
    src = open(os.path.join(ROOT, "test.py")).read()
    titles = re.findall(r'\("(MaskedL[^"]*)", MaskedL', src)
    names = re.findall(r'\("([A-Za-z_0-9]+)", (?:PowerImbalance|Masked_L2_loss|MSELoss)\(', src)
    assert titles == ["MaskedL2", "MaskedL2(denorm)", "MaskedL1(denorm)"] and names == ["PowerImbalance", "Masked_L2_loss", "MSE"]
    o = torch.zeros(2, 4)
    term_keys = list(MaskedL2V2()(o, o, torch.ones(2, 4)))
    assert term_keys == list(MaskedL1()(o, o, torch.ones(2, 4)))
    lines = [f"{t} {k}" for t in titles for k in term_keys]
    for n in names:
        lines.append(n)
        if n == "PowerImbalance":
            lines.append(f"{n}(ref)")
    assert report_keys() == lines
    assert "evaluate_report" in src and "--per-metric-passes" in src


def test_term_table_matches_the_header():
    text = open(os.path.join(ROOT, "include", "pfn_hip.h")).read()
    body = re.search(r"enum pfn_eval_term \{(.*?)\};", text, flags=re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.replace("\n", " ").split(",") if n.strip()]
    assert names[-1] == "PFN_EVAL_N_TERMS"
    assert [n[len("PFN_EVAL_"):].lower() for n in names[:-1]] == list(L.EVAL_TERMS)
    assert L.EVAL_ACC_DOUBLES == len(L.EVAL_TERMS) + 1
    assert re.search(r"#define PFN_EVAL_ACC_BATCHES PFN_EVAL_N_TERMS\b", text)
    assert L.EVAL_WS_FLOATS * 4 == 26 * 256 * 4 + 16                   # struct EvalWs of csrc/eval.hip, as the header states
    assert ">= 26640 bytes" in text and "pfn_eval_metrics" in L.SYMBOLS and "pfn_eval_accumulate" in L.SYMBOLS


def test_running_sum_on_the_host_keeps_the_reference_arithmetic():
    """Host tensors (no device): sum of value.item() * len(data), the first batch unweighted on request -- the loops' old code."""
    vals = [torch.tensor(0.1234567), torch.tensor(3.25e-5), torch.tensor(7.0e3)]
    s, want = _RunningSum(), 0.0
    for v in vals:
        s.add(v, 8)
        want += v.item() * 8
    assert s.value() == want
    s2 = _RunningSum(first_unweighted=True)
    for v in vals:
        s2.add(v, 8)
    assert s2.value() == vals[0].item() + vals[1].item() * 8 + vals[2].item() * 8
