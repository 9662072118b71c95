"""The reference's GCN baseline (`networks/GCN.py:5-21`) and the PyG layer it is made of, on the HIP kernels of csrc/gcn.hip.

  * `GCNConv(in_channels, out_channels, bias=True)` -- torch_geometric.nn.GCNConv with its defaults (self loops, symmetric
    normalisation, bias, flow source -> target): state_dict keys `lin.weight` (out, in) and `bias`, glorot / zeros initialisation.
  * `GCN(nfeature_dim, output_dim, hidden_dim, **kwargs)` -- three of them, ReLU after the first two.

The layer uses `edge_index` AS STORED (adjacency mode 0): the reference's `GCN.forward` hands `data.edge_index` to the layers
without undirecting it, and so does this.  There is no CPU implementation: host tensors raise RuntimeError.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import _lib as L
from .MPN import GraphCSR, _GraphCache, _pad_rows, _padded, _unpad_rows


class _GcnConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, graph: GraphCSR, dims, holder, x, weight, bias):
        lib = L.load()
        cin, cout, relu = dims
        n = x.shape[0]
        xp = _pad_rows(x, cin)
        out = torch.empty(n, _padded(cout), dtype=torch.float32, device=x.device)
        nbytes = lib.pfn_gcn_conv_workspace_bytes(n, graph.e_stored, cin, cout)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        L.check(lib.pfn_gcn_conv_forward(graph.ws.data_ptr(), n, graph.e_stored, cin, cout, xp.data_ptr(), _padded(cin),
                                         weight.data_ptr(), L.ptr(bias), relu, out.data_ptr(), _padded(cout), ws.data_ptr(), nbytes,
                                         L.stream_ptr()), "pfn_gcn_conv_forward")
        ctx.graph, ctx.dims, ctx.ws, ctx.has_bias = graph, dims, ws, bias is not None
        if holder is not None:
            holder._last_ws = (ws, n)              # (what export_gates reads: the decisions lead the layer's workspace)
        ctx.save_for_backward(xp, weight)
        return _unpad_rows(out, cout)

    @staticmethod
    def backward(ctx, gout):
        lib = L.load()
        cin, cout, relu = ctx.dims
        xp, weight = ctx.saved_tensors
        graph, n = ctx.graph, xp.shape[0]
        gp = _pad_rows(L.f32c(gout, "grad_out"), cout)
        gx = torch.empty_like(xp) if ctx.needs_input_grad[3] else None
        gw = torch.empty_like(weight)
        gb = torch.empty(cout, dtype=torch.float32, device=xp.device) if ctx.has_bias else None
        L.check(lib.pfn_gcn_conv_backward(graph.ws.data_ptr(), n, graph.e_stored, cin, cout, xp.data_ptr(), _padded(cin),
                                          weight.data_ptr(), gp.data_ptr(), _padded(cout), relu, L.ptr(gx), _padded(cin),
                                          gw.data_ptr(), L.ptr(gb), ctx.ws.data_ptr(), ctx.ws.numel(), L.stream_ptr()),
                "pfn_gcn_conv_backward")
        return None, None, None, (_unpad_rows(gx, cin) if gx is not None else None), gw, gb


class GCNConv(nn.Module):
    """PyG `GCNConv(in_channels, out_channels)` with its defaults:
    out_i = dis_i (sum_{e: dst = i, src != i} dis_src H_src + dis_i H_i) + b,  H = x W^T,  dis = (1 + in-degree without self
    edges)^-1/2.  Stored self edges are replaced by the one unit self loop every node gets; parallel lines count once each."""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self._graphs = _GraphCache()
        self._last_ws = None
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))      # glorot, as PyG's Linear(weight_initializer='glorot')
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index):
        L.require_device(x, edge_index, *self.parameters(), what="GCNConv input")
        with torch.cuda.device(x.device):
            graph = self._graphs.get(edge_index, x.shape[0], 0)           # the layer takes the list as given
            return self.on_graph(graph, x)

    def on_graph(self, graph: GraphCSR, x, relu=False):
        """The layer over an adjacency that is already built (mode 0); `relu=True` fuses the caller's ReLU into the launch."""
        L.require_device(x, *self.parameters(), what="GCNConv input")
        x = L.f32c(x, "x")
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"x must be (N, {self.in_channels}), got {tuple(x.shape)}")
        if graph.mode != 0:
            raise RuntimeError("GCNConv needs an adjacency built with mode 0 (the stored list, not undirected)")
        with torch.cuda.device(x.device):
            return _GcnConvFn.apply(graph, (self.in_channels, self.out_channels, 1 if relu else 0), self, x, self.lin.weight, self.bias)

    def export_gates(self) -> torch.Tensor:
        """[N, out_channels] uint8: the ReLU decisions of the last `on_graph(..., relu=True)` call (1 = on)."""
        if self._last_ws is None:
            raise RuntimeError("GCNConv.export_gates: no forward has run")
        ws, n = self._last_ws
        ld = _padded(self.out_channels)
        return ws[: n * ld].view(n, ld)[:, : self.out_channels].clone()


def _with_mask_input(data, with_mask: bool):
    """The layer input of a baseline: `data.x`, or cat[data.x, data.pred_mask.float()] (`with_mask`)."""
    if not with_mask:
        return data.x
    L.require_device(data.x, data.pred_mask, what="baseline input")
    return torch.cat([data.x.float(), data.pred_mask.float()], dim=1)


class GCN(nn.Module):
    """networks/GCN.py:5-21: conv1 -> ReLU -> conv2 -> ReLU -> conv3 over `data.x` and `data.edge_index` as stored.  The ReLUs
    run inside the layers' launches and ONE adjacency per forward serves the three layers.

    `with_mask=True` (swallowed by the reference's `**kwargs`; default False = the reference's dataflow): the input is
    cat[data.x, data.pred_mask.float()] -- pass nfeature_dim = 8.  The reference baseline was written for the 16-wide node layout
    that carried the mask columns; with today's 4-wide x a baseline cannot tell a zeroed entry from an unknown one without it."""

    def __init__(self, nfeature_dim, output_dim, hidden_dim, **kwargs):
        super().__init__()
        self.with_mask = bool(kwargs.get("with_mask", False))
        self.nfeature_dim, self.output_dim, self.hidden_dim = nfeature_dim, output_dim, hidden_dim
        self.conv1 = GCNConv(nfeature_dim, hidden_dim)
        self.conv2 = GCNConv(hidden_dim, hidden_dim)
        self.conv3 = GCNConv(hidden_dim, output_dim)
        self.relu = nn.ReLU()                          # (kept for the reference's attribute surface; the ReLUs are fused)
        self._graphs = _GraphCache()

    def forward(self, data):
        L.require_device(data.x, data.edge_index, *self.parameters(), what="GCN input")
        x = _with_mask_input(data, self.with_mask)
        with torch.cuda.device(x.device):
            graph = self._graphs.get(data.edge_index, x.shape[0], 0)
            x = self.conv1.on_graph(graph, x.float(), relu=True)
            x = self.conv2.on_graph(graph, x, relu=True)
            return self.conv3.on_graph(graph, x)

    def export_gates(self):
        """The two hidden layers' ReLU decisions of the last forward, each [N, hidden_dim] uint8 (1 = on)."""
        return [self.conv1.export_gates(), self.conv2.export_gates()]
