"""Host logic without a GPU: argument parser precedence, loss dispatch helpers, train/eval loop semantics (driven with
the CPU oracle model, which is allowed in tests), and the world-size-2 gloo data-parallel step."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import ref_cpu
from poweflownet_amd import dp
from poweflownet_amd.data import DataLoader
from poweflownet_amd.synth import make_batch, make_dataset
from poweflownet_amd.utils.argument_parser import argument_parser
from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss, PowerImbalance
from poweflownet_amd.utils.evaluation import evaluate_epoch, num_params
from poweflownet_amd.utils.training import train_epoch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_parser_precedence():
    a = argument_parser(["--cfg_json", os.path.join(ROOT, "configs", "wide.json"), "--case", "6470rte", "--K", "5"])
    assert (a.hidden_dim, a.n_gnn_layers, a.K, a.case) == (129, 6, 5, "6470rte")      # defaults < JSON < CLI
    b = argument_parser([])                  # like the reference, no flag = configs/standard.json (hidden_dim 129)
    assert (b.hidden_dim, b.train_loss_fn, b.batch_size, b.cfg_json) == (129, "masked_l2", 128, "configs/standard.json")


class OracleMaskedL2(Masked_L2_loss):
    """The product's Masked_L2_loss has no CPU path; the host-logic tests below run the loops on the CPU oracle model, so
    they use the oracle's restatement of the loss behind the SAME class (the loops dispatch on isinstance)."""

    def forward(self, output, target, mask):
        return ref_cpu.masked_l2_loss(output, target, mask, self.regularize, self.regcoeff)


def test_losses_have_no_cpu_path():
    torch.manual_seed(0)
    out, y = torch.randn(10, 4), torch.randn(10, 4)
    mask = torch.randint(0, 2, (10, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        Masked_L2_loss(regularize=True, regcoeff=0.5)(out, y, mask)
    from poweflownet_amd.loss import MSELoss
    with pytest.raises(RuntimeError, match="HIP device"):
        MSELoss()(out, y)
    pi = PowerImbalance(torch.zeros(1, 4), torch.ones(1, 4), torch.zeros(1, 2), torch.ones(1, 2))
    with pytest.raises(RuntimeError):
        pi(out, torch.zeros(2, 3, dtype=torch.long), torch.randn(3, 2))


def test_train_and_eval_epoch_semantics_on_oracle_model():
    torch.manual_seed(0)
    ds = make_dataset("14", 12)
    loader = DataLoader(ds, batch_size=4)
    model = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 16, 2, 2, 0.0)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    before = evaluate_epoch(model, loader, OracleMaskedL2(regularize=False), "cpu")
    l1 = train_epoch(model, loader, torch.nn.MSELoss(), opt, "cpu")
    l2 = train_epoch(model, loader, OracleMaskedL2(), opt, "cpu")
    for _ in range(20):
        l2 = train_epoch(model, loader, OracleMaskedL2(), opt, "cpu")
    after = evaluate_epoch(model, loader, OracleMaskedL2(regularize=False), "cpu")
    assert l1 > 0 and l2 > 0 and after < before
    assert num_params(model) == sum(p.numel() for p in model.parameters())


def _dp_worker(rank, world, port, ret):
    # a host-only rank (gloo, CPU tensors): on a box with fewer GPUs than ranks, init_from_env must not select device `rank`
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), PFN_SINGLE_DEVICE="1")
    torch.set_num_threads(1)
    r, _, w = dp.init_from_env(backend="gloo")
    ds = make_dataset("14", 8)
    torch.manual_seed(1234 + rank)                       # deliberately different init: broadcast must fix it
    model = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 8, 2, 3, 0.0)
    dp.broadcast_parameters(model)
    loader = DataLoader(ds, batch_size=8, shard=(r, w))
    batch = next(iter(loader))
    loss = torch.nn.MSELoss()(model(batch), batch.y)
    loss.backward()
    dp.allreduce_gradients(model, ordered_params=list(model.parameters()))
    flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    if rank == 0:
        ret["grad"], ret["params"] = flat.clone(), params.clone()
    gathered = [torch.zeros_like(flat) for _ in range(w)]
    dist.all_gather(gathered, flat)
    assert all(torch.equal(g, gathered[0]) for g in gathered)
    dist.destroy_process_group()


def test_dp_world2_gloo_equals_single_process_global_batch():
    """Mean of the two ranks' gradients on their shards == gradient on the global batch (MSELoss mean, equal node counts)."""
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_dp_worker, args=(2, port, ret), nprocs=2, join=True)
    torch.set_num_threads(1)
    ds = make_dataset("14", 8)
    torch.manual_seed(1234)
    model = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 8, 2, 3, 0.0)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in model.parameters()]), ret["params"])
    batch = next(iter(DataLoader(ds, batch_size=8)))
    torch.nn.MSELoss()(model(batch), batch.y).backward()
    want = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    got = ret["grad"]
    assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item() + 1e-9


def _agree_worker(rank, w, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=w)
    from poweflownet_amd import dp
    calls = []
    gs = dp.GraphedStep(lambda: calls.append("fb") or torch.zeros(()), lambda: calls.append("opt"), model=None, allreduce=True, mode="graph")
    gs._reduce = lambda: calls.append("reduce")
    gs._reduce_captured = gs._reduce
    # a capture attempt that fails on rank 1 ONLY: every rank must report failure (and then agree on the next form)
    def build():
        if rank == 1:
            raise RuntimeError("capture failed here")
        gs.graphs = ["a graph"]
    ok_mixed = gs._try(build)
    ok_all = gs._try(lambda: None)
    # no GPU in this process: both graph forms fail on every rank -> everybody lands in "eager", whose replay is the three calls
    gs.capture()
    gs.replay()
    ret[rank] = (ok_mixed, ok_all, gs.form, list(gs.graphs), calls[-3:])
    dist.destroy_process_group()


def test_dp_ranks_agree_on_the_launch_form():
    """dp.GraphedStep: a capture that fails on ONE rank demotes EVERY rank (the success flag is MIN-all-reduced before a form is
    chosen), so ranks never disagree on how a step is launched; world 2 over gloo, no GPU: both graph forms fail everywhere and
    the step runs as eager launches (fwd_bwd, all-reduce, optimizer)."""
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_agree_worker, args=(2, port, ret), nprocs=2, join=True)
    for rank in (0, 1):
        ok_mixed, ok_all, form, graphs, calls = ret[rank]
        assert ok_mixed is False and ok_all is True and form == "eager" and graphs == [] and calls == ["fb", "reduce", "opt"], (rank, ret[rank])


def test_evaluation_metrics_and_evaluate_epoch_v2():
    """MaskedL2V2 / MaskedL1 (reference utils/custom_loss_functions.py:48-97) by their definitions, and evaluate_epoch_v2's
    accumulation rule (utils/evaluation.py:158-165: first batch unweighted, the rest weighted by len(data))."""
    from poweflownet_amd.utils.custom_loss_functions import MaskedL1, MaskedL2V2
    from poweflownet_amd.utils.evaluation import evaluate_epoch_v2
    torch.manual_seed(1)
    out, y = torch.randn(30, 4), torch.randn(30, 4)
    mask = torch.randint(0, 2, (30, 4))
    for cls, err in ((MaskedL2V2, (out - y) ** 2), (MaskedL1, (out - y).abs())):
        t = cls()(out, y, mask)
        per = torch.stack([err[:, f][mask[:, f].bool()].mean() for f in range(4)])
        assert torch.allclose(torch.stack([t["vm"], t["va"], t["p"], t["q"]]), per, atol=1e-6)
        assert torch.allclose(t["balanced total"], per.mean(), atol=1e-6)
        assert torch.allclose(t["total"], err[mask.bool()].mean(), atol=1e-6)

    class Echo(torch.nn.Module):             # "model" whose prediction is its input
        def forward(self, data):
            return data.x

    batches = [make_batch("14", b, seed=b) for b in (2, 3, 1)]
    got = evaluate_epoch_v2(Echo(), batches, MaskedL2V2(), "cpu")
    terms = [MaskedL2V2()(b.x, b.y, b.pred_mask) for b in batches]
    lens = [len(b) for b in batches]
    want = (terms[0]["total"].item() + sum(t["total"].item() * n for t, n in zip(terms[1:], lens[1:]))) / sum(lens)
    assert abs(got["total"] - want) < 1e-6 and set(got) == {"total", "balanced total", "vm", "va", "p", "q"}


def test_gemm_nt_block_order_covers_every_row_group_and_slice_once():
    """gemm_nt_kernel reads its launch-order id as [chunk of 8 row groups][slice][row group in chunk] so that the column slices of a
    row group share an XCD (csrc/gemm_nt.hip, round 6; a tail of gx % 8 row groups keeps the plain order).  The mapping restated here
    line by line must be a bijection onto (row group, slice) for every grid the launcher can produce, and must put the slices of a
    row group of a full chunk on launch ids that are equal modulo 8 (= the same XCD under round-robin dispatch)."""
    import re
    src = open(os.path.join(ROOT, "poweflownet_amd", "csrc", "gemm_nt.hip")).read()
    # (the test follows the source: if these lines change, restate the mapping below)
    for line in ("const int chunk = lin / (8 * ns), r = lin - chunk * 8 * ns;", "slice = r >> 3;", "bx = chunk * 8 + (r & 7);",
                 "const int t = lin - full * ns, tail = gx - full;", "slice = t / tail;", "bx = full + (t - slice * tail);"):
        assert line in src, line
    assert re.search(r"full = gx & ~7", src)

    def block_of(lin, gx, ns):
        full = gx & ~7
        if ns > 1 and lin < full * ns:
            chunk, r = divmod(lin, 8 * ns)
            return chunk * 8 + (r & 7), r >> 3
        if ns > 1:
            t, tail = lin - full * ns, gx - full
            s = t // tail
            return full + (t - s * tail), s
        return lin % gx, lin // gx

    for ns in (1, 2, 3, 4):
        for gx in list(range(1, 40)) + [59, 118, 120, 127, 128, 256]:
            seen = {}
            for lin in range(gx * ns):
                seen.setdefault(block_of(lin, gx, ns), []).append(lin)
            assert sorted(seen) == [(b, s) for b in range(gx) for s in range(ns)], (gx, ns)
            assert all(len(v) == 1 for v in seen.values())
            if ns > 1:
                for b in range(gx & ~7):
                    assert len({seen[(b, s)][0] % 8 for s in range(ns)}) == 1, (gx, ns, b)


# ------------------------------------------------------------------------------------------ tests/regimes.py, pinned to csrc/
REGIME_PINS = {
    # the graph-resident EdgeAggregation / seg_lin_hops / front_seg kernels
    "seg_tile.hpp": ("constexpr int SG_MAX_ROWS = 128;", "constexpr int SG_LDS_BYTES = 78 * 1024;", "constexpr int SG_NCH = 17;",
                     "constexpr int SG_TW = 36;"),
    "ea_seg.hip": ("constexpr int SG_W2A_CH = 34;",
                   "if (seg <= 0 || seg > SG_MAX_ROWS || n <= 0 || n % seg != 0) return false;",
                   "const int gpb = std::max(1, SG_MAX_ROWS / seg);", "p.trows = (p.rows_pb + 31) / 32 * 32;", "p.cap = p.rows_pb * 4;",
                   "return p.ny >= 1 && ld <= 8 * SG_NCH &&", "(!bwd_limits || p.nblocks <= 1024) &&",
                   "size_t f = (size_t)(bwd ? 3 : 2) * trows * SG_TW + (bwd ? 0 : 2 * SG_NCH * 256) + 2 * SG_TW + (bwd ? 4 * SG_TW + 4 * "
                   "SG_W2A_CH * 4 + 8 * 16 * 2 * 4 : 0) + (size_t)(bwd ? 2 : 1) * 2 * cap;",
                   "const size_t tile = (size_t)trows * SG_TW, img = (size_t)SG_NCH * 256;", "return tile > img ? tile : img;",
                   "if (bwd) f += seg_bwd_d_floats(trows) - (size_t)trows * SG_TW;",
                   "size_t i = (size_t)(bwd ? 2 : 1) * (rows_pb + 1 + cap);", "return (f + i) * 4 + 16;",
                   "const long per_cu = 4L;",
                   "return !off && fe == 2 && seg_plan(seg, n, ld, p, bwd) && (long)p.nblocks * p.ny <= per_cu * device_cus();",
                   "return !off && ld / 4 <= 64 && front_latency_regime(h, n) && ea_seg_fit(seg, n, fe, ld, false);",
                   "bool ea_seg_bwd_out_ok(int fo) { return ((fo + 7) & ~7) <= 8 * SG_NCH; }"),
    "seg_lin_hops.hip": ("const long per_cu = 4L;   // (ea_seg_fit's bound)", "fused_hops_fit(seg, ld, n) &&",
                         "slh_plan(seg, n, ld, nterm, p) && (long)p.nblocks * p.ny <= per_cu * device_cus();"),
    # (make_route: every whole-model decision, once per entry point; hop_kind: the TAGConv hop kernel)
    "model.hip": ("r.ea_seg_fwd = ea_seg_fit(seg, lo.n, lo.fe, lo.ld, false);", "r.ea_seg_bwd = ea_seg_fit(seg, lo.n, lo.fe, lo.ld, true);",
                  "if (!ea_seg_bwd_out_ok(lo.fo)) r.ea_seg_bwd = false;",
                  "const bool seg_walk = o.ea_in && o.ea_out && (fo > 4 || ldgo == 4);",
                  "const bool out_in_walk = !seg_walk && !o.walk_done && w2 && act.act == ACT_NONE && edge_fwd_out_ok(fe, h, fo, ldo) && o.back_fused;",
                  "r.seg_gates = !no_gates && train && lo.fe == 2 && r.ea_seg_fwd && r.ea_seg_bwd && (r.seg_front || !r.fused_front);",
                  "r.fused_front = front_fused_ok(lo.f0, lo.h);",
                  "const bool generic_fwd = !r.ea_seg_fwd || (r.fused_front && i == 0);",
                  "r.mask[i] = train && lo.fe == 2 && generic_fwd && !r.ea_seg_bwd;",
                  "r.l0_fly = !no_fly && r.fused_front && lo.nlayers > 1 && lo.fe == 2 && lo.f0 == 4 && !front_latency_regime(lo.h, lo.n) &&",
                  "(!train || r.mask[0]);",
                  "r.seg_front = r.fused_front && r.ea_seg_fwd && !r.l0_fly && lo.nlayers > 1 &&",
                  "front_seg_fit(seg, lo.n, lo.h, lo.fe) && !(train && lo.fe == 2 && !r.ea_seg_bwd);",
                  "const bool train = c.need_backward != 0, out4 = lin_out4_ok(lo.h, lo.fo, lo.ldo, lo.n);",
                  "r.mse_tail = !no_tail && train && lo.n > 0 && lo.nlayers > 1 && lo.fe == 2 && lo.fo == 4 && lo.ldo == 4 &&",
                  "out4 && r.back_fused && r.ea_seg_fwd && r.ea_seg_bwd && lo.ld / 4 <= 34;",
                  "r.masked_tail = r.mse_tail && r.seg_front;", "return r.masked_tail ? 1 : 0;",
                  "if (K > 0 && fused_hops_fit(seg, ld, n)) return HOPS_FUSED;", "if (K > 0 && big_hops_fit(seg, n, e_stored)) return HOPS_BIG;",
                  "r.hops = hop_kind(seg, lo.ld, lo.n, e_stored, lo.K);",
                  "r.slh_fwd = !r.big_cm && seg_lin_hops_fit(seg, lo.n, lo.ld, lo.h, lo.h, lo.K, 1);",
                  "r.slh_bwd = !r.big_cm && seg_lin_hops_fit(seg, lo.n, lo.ld, lo.h, lo.h, lo.K, 2);"),
    # the row-per-wave front and the last layer
    "front.hip": ("static int wave_max_rows() { return 32768; }",
                  "return !off && fo >= 1 && fo <= 4 && ldo == 4 && ld_of(h) / 4 <= 64 && n <= wave_max_rows();",
                  "return !off && f0 == 4 && ld_of(h) / 4 <= 256;", "return !off && nchunk <= 64 && n <= wave_max_rows();",
                  "bool front_latency_regime(int h, int n) { return front_row_per_wave(ld_of(h) / 4, n); }"),
    # TAGConv hops, edge rows
    "edge.hip": ("constexpr int FH_LDS_BYTES = 156 * 1024;",
                 "if (seg <= 0 || (size_t)2 * seg * 4 * sizeof(float) + (size_t)(2 * seg + 1) * sizeof(int) > (size_t)FH_LDS_BYTES / 2) return false;",
                 "constexpr int BH_THREADS = 1024;", "constexpr int BH_RPT = 8;", "constexpr int BH_HUB_DEG = 32;", "constexpr int BH_HUB_CAP = 128;",
                 "return (size_t)BH_HUB_CAP * 16 + (size_t)BH_HUB_CAP * 2 + 16;",
                 "if (off || seg <= 0 || n <= 0 || n % seg != 0 || seg > BH_RPT * BH_THREADS || seg >= 65536) return false;",
                 "return (size_t)(seg + 1) * 16 + bh_hub_bytes() + (size_t)((seg + 2 + 7) & ~7) * 2 + 1024 <= (size_t)160 * 1024;",
                 "if (!(ne + 4 <= nb_cap && ne < 65536)) {",
                 "const size_t fixed = (size_t)(a.seg + 1) * 16 + bh_hub_bytes() + (size_t)((a.seg + 2 + 7) & ~7) * 2;",
                 "const size_t want_nb = (size_t)(2 * (int64_t)g.e_stored / std::max(1, ngraphs) + 64) * 2;",
                 "const size_t lds_total = std::min((size_t)160 * 1024, fixed + want_nb);",
                 "const int nb_cap = (int)((lds_total - fixed) / 2);",
                 "if (cnt > BH_HUB_DEG && rowu < seg) {", "if (sl < BH_HUB_CAP) {", "((uint32_t)min(cnt, 255) << 16)",
                 "constexpr int RH_THREADS = 512;", "constexpr int RH_IPT = 8;", "constexpr int ER_THREADS = 512;", "constexpr int ER_IPT = 8;",
                 "if (seg <= 0 || seg > 1023 || (long)seg * nchunk > (long)RH_IPT * RH_THREADS) return 0;",
                 "int gpb = std::min((RH_IPT * RH_THREADS) / (seg * nchunk), 1023 / seg);",
                 "while (gpb > 0 && (size_t)gpb * seg * nchunk * 16 + (size_t)((gpb * seg + 2 + 7) & ~7) * 2 + 4096 > (size_t)78 * 1024) --gpb;",
                 "if (!off && !a.transpose && gpb > 0 && (long)(ngraphs + gpb - 1) / gpb >= 4L * device_cus()) {",
                 "if (seg <= 0 || seg > 1023 || (long)seg * nchunk > (long)ER_IPT * ER_THREADS || 8 * nchunk > ER_THREADS) return 0;",
                 "int gpb = std::min((ER_IPT * ER_THREADS) / (seg * nchunk), 1023 / seg);",
                 "while (gpb > 0 && (size_t)gpb * seg * nchunk * 16 + 4096 > (size_t)66 * 1024) --gpb;",
                 "if (!off && gpb > 0 && (long)(ngraphs + gpb - 1) / gpb >= 4L * device_cus()) {",
                 "bool edge_fwd_out_ok(int fe, int h, int fo, int ldo) { return fe == 2 && fo >= 1 && fo <= 4 && ldo == 4 && ld_of(h) / 4 <= 256; }"),
    # the TAGConv products
    "gemm_nt.hip": ("constexpr int NT_THREADS = 512;", "constexpr int NCH = 17;", "constexpr int KP = 8 * NCH;", "constexpr int NT_MAX_PIECES = 16;",
                    "constexpr int NT_LDS_BYTES = 160 * 1024;", "constexpr int TINY_MAX_PIECES = 8;",
                    'atoi(diag_env("PFN_NT_TINY_MAX_TILES")) : 256;', 'atoi(diag_env("PFN_NT_WS_MIN_TILES")) : 2;',
                    "bool tiny_ok = tiny_max > 0 && nrt <= tiny_max && nq == 4 && remv == 4 && nrem == 1 &&",
                    "pieces.size() <= (size_t)TINY_MAX_PIECES",
                    "const long per_round = (long)ncu * NT_WAVES;",
                    "bool ws_ok = ws_min > 0 && nq == 4 && remv == 4 && nrem == 1 && nslices > 2 && pieces.size() <= (size_t)NT_MAX_PIECES &&",
                    "(long)nrt >= (long)ws_min * per_round;", "const long nround = nrt / per_round;",
                    "const long rows_ws = std::min<long>(a.M, nround * per_round * 32);",
                    "bool wide_ok = remv == 0 && nq >= 8 && nq % 4 == 0 && pieces.size() <= (size_t)NT_MAX_PIECES && a.ldc == 32 * nq;",
                    "if (fast && tps >= 2 && (long)nrt * nslices * (tps / 2) >= 2L * ncu * NT_WAVES) CT = 2;",
                    "if (tot <= lds_budget && pieces.size() <= (size_t)NT_MAX_PIECES) break;"),
    "pfn_internal.hpp": ("remv = (m != 0 && m <= 4) ? m : 0;", "nq = (ld - remv + 31) / 32;", "static inline int ld_of(int f) { return (int)round_up(f, 4); }"),
}


def regime_pin_failures(csrc):
    """(file, line) of every pinned line that is no longer in `csrc` (whitespace runs compared as one blank)."""
    import re
    missing = []
    for name, lines in REGIME_PINS.items():
        src = re.sub(r"\s+", " ", open(os.path.join(csrc, name)).read())
        missing += [(name, ln) for ln in lines if re.sub(r"\s+", " ", ln) not in src]
    return missing


def test_regime_constants_are_still_in_the_source():
    """tests/regimes.py restates the dispatch predicates of the forward and backward passes (tests/test_gpu_boundaries.py picks
    the shapes on both sides of every edge from it).  Every constant and formula it restates must still be written in csrc/,
    literally: a threshold that moves fails here, on the CPU, before the GPU tests straddle the wrong place."""
    from tests import regimes as R
    assert regime_pin_failures(os.path.join(ROOT, "poweflownet_amd", "csrc")) == []
    # the restatement's own constants are the pinned ones
    assert (R.SG_MAX_ROWS, R.SG_LDS_BYTES, R.SG_NCH, R.SG_TW, R.SG_W2A_CH, R.SG_BWD_MAX_BLOCKS, R.PER_CU) == (128, 78 * 1024, 17, 36, 34, 1024, 4)
    assert (R.WAVE_MAX_ROWS, R.FH_LDS_BYTES, R.BH_RPT, R.BH_THREADS, R.BH_HUB_DEG, R.BH_HUB_CAP) == (32768, 156 * 1024, 8, 1024, 32, 128)
    assert (R.RH_THREADS, R.RH_IPT, R.ER_THREADS, R.ER_IPT) == (512, 8, 512, 8)
    assert (R.NT_THREADS, R.NCH, R.KP, R.NT_MAX_PIECES, R.NT_LDS_BYTES, R.TINY_MAX_PIECES, R.TINY_MAX_TILES, R.WS_MIN_ROUNDS) == \
        (512, 17, 136, 16, 160 * 1024, 8, 256, 2)


def test_route_invariants_hold_over_a_sweep_of_models_and_batches():
    """csrc/model.hip make_route ends with a check of what the passes take for granted of each other (the graph-resident backward
    reads what the graph-resident forward filled, front_seg_fwd_kernel never runs where layer 0's backward reads ReLU masks, ...) and
    refuses the call if it fails.  Each implication follows from the predicates: swept here over their restatement -- CU counts,
    hidden widths, graph sizes and graph counts on both sides of every threshold, training and inference -- so the check can never
    refuse a valid call, and a predicate edited into contradiction with another fails on the CPU."""
    import re
    from tests import regimes as R
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "poweflownet_amd", "csrc", "model.hip")).read())
    for clause in ("(!r.ea_seg_bwd || r.ea_seg_fwd)", "(!r.seg_front || !r.mask[0])", "(!r.l0_fly || (r.fused_front && !r.seg_front))",
                   "(!r.meh_recompute || r.l0_fly)", "(!r.mse_tail || (r.ea_seg_fwd && r.ea_seg_bwd && out4))",
                   "(!(r.slh_fwd || r.slh_bwd) || (r.hops == HOPS_FUSED && !r.big_cm))", "(!r.big_cm || r.hops == HOPS_BIG)"):
        assert clause in src, clause
    count = 0
    for cus in (32, 64, 256, 304):
        for H in (8, 16, 64, 128, 129, 136, 256, 257, 512):
            for seg in (1, 2, 14, 30, 118, 127, 128, 129, 300, 1023, 1024, 1996, 1997, 2500, 6470, 8192, 8193):
                for B in (1, 2, 8, 9, 37, 128, 277, 278, 1024, 2048, 2171, 33000):
                    for train in (False, True):
                        for L, K in ((2, 1), (4, 3), (4, 6), (2, 6)):
                            r = R.route(seg * B, seg, H, L, K, 2, train, cus)
                            assert R.route_contradictions(r) == [], (cus, H, seg, B, train, L, K, r)
                            count += 1
    assert count == 4 * 9 * 17 * 12 * 2 * 4
    # ... and over the output width: the last layer's dS product is one k piece up to fo = 136 (ea_seg_bwd_out_ok); a wider output
    # pairs the graph-resident forward with the generic backward, which must leave every other decision consistent
    assert [R.ea_seg_bwd_out_ok(fo) for fo in (1, 3, 4, 5, 136, 137, 200)] == [True] * 5 + [False] * 2
    count = 0
    for fo in (1, 3, 4, 5, 136, 137, 200):
        for cus in (32, 256):
            for H in (3, 7, 16, 33, 64, 65, 129, 136, 137, 256):
                for seg in (1, 14, 118, 128, 129, 1996, 1997, 8193):
                    for B in (1, 2, 6, 37, 278, 2341, 33000):
                        for train in (False, True):
                            for fe in (1, 2, 6):
                                for L, K in ((2, 0), (3, 2), (2, 3)):
                                    n = seg * B
                                    r = R.route(n, seg, H, L, K, fe, train, cus, fo=fo)
                                    assert R.route_contradictions(r) == [], (fo, cus, H, seg, B, train, fe, L, K, r)
                                    # the clause itself, and what follows from the existing lines: no gates, no graph-resident
                                    # front, no loss tail without the graph-resident backward
                                    assert r["ea_seg_bwd"] == (R.ea_seg_fit(seg, n, fe, R.ld_of(H), True, cus) and fo <= 136)
                                    if train and fe == 2 and not r["ea_seg_bwd"]:
                                        assert not r["seg_gates"] and not r["seg_front"] and not r["mse_tail"]
                                        assert r["mask0"] == (not r["ea_seg_fwd"] or r["fused_front"]) and r["mask1"] == (not r["ea_seg_fwd"])
                                    assert r["mse_tail"] <= (fo == 4) and r["lin_out4"] <= (fo <= 4)
                                    reg = R.model_regime(n, seg, H, L, K, fe, train, cus, fo=fo)
                                    assert not (reg["must"] & reg["must_not"]), (fo, cus, H, seg, B, train, fe, L, K, reg)
                                    if fo == 4:       # the keyword's default is the old restatement
                                        assert r == R.route(n, seg, H, L, K, fe, train, cus)
                                        assert reg == R.model_regime(n, seg, H, L, K, fe, train, cus)
                                    count += 1
    assert count == 7 * 2 * 10 * 8 * 7 * 2 * 3 * 3
    # the check itself: a route with one decision flipped is refused
    r = R.route(118 * 128, 118, 129, 4, 3, 2, True, 256)
    assert r["mse_tail"] and r["seg_front"] and r["slh_fwd"] and R.route_contradictions(r) == []
    for key, value in (("ea_seg_fwd", False), ("mask0", True), ("l0_fly", True), ("hops", "generic"), ("big_cm", 118 * 128)):
        assert R.route_contradictions(dict(r, **{key: value})) != [], key
    # the wide output at the flagship batch: forward graph-resident, backward generic, layer 0's masks saved by its generic walk
    for fo, bwd in ((136, True), (137, False), (200, False)):
        r = R.route(118 * 128, 118, 129, 4, 3, 2, True, 256, fo=fo)
        assert r["ea_seg_fwd"] and r["ea_seg_bwd"] == bwd and r["seg_gates"] == bwd and r["seg_front"] == bwd and r["mask0"] == (not bwd)
        reg = R.model_regime(118 * 128, 118, 129, 4, 3, 2, True, 256, fo=fo)
        assert ("ea_seg_bwd" in reg["must"]) == bwd and ("edge_bwd" in reg["must"]) == (not bwd)
        assert ("ea_seg_bwd" in reg["must_not"]) == (not bwd)


def test_regime_pins_fail_on_a_moved_threshold(tmp_path):
    """The pin check itself: a copy of csrc/ with one threshold moved (SG_MAX_ROWS, per_cu, wave_max_rows, FH_LDS_BYTES, BH_RPT,
    BH_HUB_CAP, the tiny / streaming defaults, NT_MAX_PIECES, TINY_MAX_PIECES) must fail it."""
    import shutil
    csrc = os.path.join(ROOT, "poweflownet_amd", "csrc")
    moves = [("seg_tile.hpp", "SG_MAX_ROWS = 128", "SG_MAX_ROWS = 129"), ("ea_seg.hip", "per_cu = 4L", "per_cu = 8L"),
             ("seg_lin_hops.hip", "per_cu = 4L", "per_cu = 2L"), ("front.hip", "return 32768;", "return 32767;"),
             ("edge.hip", "FH_LDS_BYTES = 156 * 1024", "FH_LDS_BYTES = 160 * 1024"), ("edge.hip", "BH_RPT = 8;", "BH_RPT = 9;"),
             ("edge.hip", "BH_HUB_CAP = 128;", "BH_HUB_CAP = 64;"), ("gemm_nt.hip", "TINY_MAX_TILES\")) : 256;", "TINY_MAX_TILES\")) : 255;"),
             ("gemm_nt.hip", "WS_MIN_TILES\")) : 2;", "WS_MIN_TILES\")) : 3;"), ("gemm_nt.hip", "NT_MAX_PIECES = 16;", "NT_MAX_PIECES = 12;"),
             ("gemm_nt.hip", "TINY_MAX_PIECES = 8;", "TINY_MAX_PIECES = 7;"), ("seg_tile.hpp", "SG_LDS_BYTES = 78 * 1024", "SG_LDS_BYTES = 80 * 1024")]
    for name, old, new in moves:
        work = tmp_path / "csrc"
        if work.exists():
            shutil.rmtree(work)
        work.mkdir()
        for f in REGIME_PINS:
            shutil.copy(os.path.join(csrc, f), work / f)
        text = (work / name).read_text()
        assert text.count(old) >= 1, (name, old)
        (work / name).write_text(text.replace(old, new))
        assert regime_pin_failures(str(work)) != [], (name, old, new)


def test_regime_restatement_agrees_with_what_the_gpu_tests_assert():
    """The restated predicates (256 CUs, the MI355X the existing GPU tests were written against) give the regimes those tests
    assert from the profile classes or the segment check."""
    from tests import regimes as R
    cus = 256
    # tests/test_gpu_mse_tail.py: the attached tail at 118v2 x 128, 118v2 x 16, 14 x 37, 14 x 300 (H 129, L 4); not at 118v2 x 2048
    for seg, B in ((118, 128), (118, 16), (14, 37), (14, 300), (118, 32), (118, 8)):
        assert R.mse_tail_available(True, seg * B, 129, 4, 2, seg, cus), (seg, B)
        r = R.model_regime(seg * B, seg, 129, 4, 3, 2, True, cus)
        assert r["seg_front"] and r["ea_seg_bwd"] and r["slh"] and "front_seg_fwd+pack" in r["must"], (seg, B)
    assert not R.mse_tail_available(True, 118 * 2048, 129, 4, 2, 118, cus)
    r = R.model_regime(118 * 2048, 118, 129, 4, 3, 2, True, cus)
    assert not r["ea_seg_fwd"] and not r["seg_front"] and "edge_bwd" in r["must"] and "ea_seg_bwd+out+mse" in r["must_not"]
    # test_fused_lds_hops_match_generic_path: 118 x 6 and 14 x 37 take the graph-resident kernels and the fused LDS hops
    for seg, B in ((118, 6), (14, 37)):
        assert R.ea_seg_fit(seg, seg * B, 2, 132, False, cus) and R.hop_kernel(seg, seg * B, 3) == "fused"
    # the big-graph tests: 2,500- and 6,470-node grids take big_graph_hops_kernel, never the two-tile one
    for seg in (2500, 6470):
        assert R.hop_kernel(seg, seg * 4, 6) == "big" and not R.fused_hops_fit(seg)
    # test_train_mode_matches_oracle_fed_the_exported_masks / test_wide_k6_large_batch_streaming_gemm_vs_oracle: K = 6 at 1,152
    # 118-bus graphs = 135,936 rows: the 7-term TAGConv products stream over whole rounds, the stationary kernel takes the tail
    plan = R.gemm_nt_plan(118 * 1152, 129, 129, 7, cus)
    assert plan["kind"] == "ws+stationary" and plan["rows_ws"] == 2 * cus * 8 * 32, plan
    # the thresholds of the issue's table at 256 CUs
    first_out = {(seg, H): R.first_graph_count(lambda b: not R.ea_seg_fit(seg, seg * b, 2, R.ld_of(H), False, cus))
                 for seg, H in ((118, 129), (14, 129), (118, 32))}
    assert first_out == {(118, 129): 257, (14, 129): 2305, (118, 32): 1025}
    assert max(s for s in range(1, 5000) if R.fused_hops_fit(s)) == 1996
    assert max(s for s in range(1, 20000) if R.big_hops_fit(s, s)) == 8192
    # big_graph_hops_kernel's staging: nb_cap is what decides; its `ne < 65536` clause cannot (nb_cap <= 62,776 for seg >= 1,997)
    assert max(R.big_hops_nb_cap(s, s, 1 << 40) for s in range(1997, 8193)) == 62776
    assert R.big_hops_nb_cap(2000, 4000, 1 << 40) == 62744 and R.big_hops_nb_cap(8000, 16000, 54000) == 8744
    assert R.big_hops_staged(2000, 4000, 2 * 62740, 62740) and not R.big_hops_staged(2000, 4000, 2 * 62741, 62741)
    assert R.big_hops_staged(8192, 16384, 14000, 7000) and not R.big_hops_staged(8192, 16384, 2 * 24576, 24576)
    assert [R.gemm_nt_plan(M, 129, 129, 4, cus)["kind"] for M in (8192, 8193, 8224)] == ["tiny", "stationary", "stationary"]
    assert [R.gemm_nt_plan(M, 129, 129, 5, cus)["kind"] for M in (131040, 131041, 131072, 131073, 196641)] == \
        ["stationary", "ws", "ws", "ws+stationary", "ws+stationary"]
    assert [R.gemm_nt_plan(1000, ci, co, K + 1, cus)["kind"] for ci, co, K in ((512, 512, 3), (512, 512, 7), (300, 129, 7))] == \
        ["wide", "multi", "multi"]
    assert [R.gemm_nt_plan(M, 129, 129, 2, cus)["CT"] for M in (65504, 65505)] == [1, 2]
