"""The reference's MLP baseline (`networks/MLP.py:4-30`) with its Linears on the HIP GEMM.

Same constructor, attribute names and state_dict keys (`layers.{i}.weight` / `.bias`).  ReLU and `nn.Dropout` are torch device
ops (there is no stream parity claim for the dropout mask).  There is no CPU implementation: host tensors raise RuntimeError.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _lib as L
from .GCN import _with_mask_input
from .MPN import _GraphCache, _hip_linear


class MLP(nn.Module):
    """MLP(input_dim, output_dim, hidden_dim, num_layers, dropout_rate): Linear(input, hidden), num_layers - 1 times
    Linear(hidden, hidden), Linear(hidden, output); ReLU and Dropout after all but the last.

    `forward(data)` flattens every graph of the batch into one row, `data.x.float().view(-1, input_dim)` (input_dim = buses x
    features of ONE grid), and returns one row per node, `.view(data.x.shape[0], -1)`.  The reference ends with `.view(-1, 6)`:
    the same thing in its stale 6-column node layout (output_dim = buses x 6 there); with today's 4 target columns it is
    `.view(-1, 4)`, which is what one row per node gives.

    `with_mask=True`: the input is cat[data.x, data.pred_mask.float()] per node (input_dim = buses x 8), see `GCN`.

    The first Linear's width is the whole grid (6470rte: 25 880 inputs).  Where the GEMM entry point rejects a width, the forward
    raises a RuntimeError that says so; the GEMM is not widened for the baseline."""

    def __init__(self, input_dim, output_dim, hidden_dim, num_layers, dropout_rate, with_mask=False):
        super().__init__()
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.output_dim = output_dim
        self.num_layers = num_layers
        self.dropout_rate = dropout_rate
        self.with_mask = bool(with_mask)

        self.layers = nn.ModuleList()
        self.layers.append(nn.Linear(input_dim, hidden_dim))
        for _ in range(num_layers - 1):
            self.layers.append(nn.Linear(hidden_dim, hidden_dim))
        self.layers.append(nn.Linear(hidden_dim, output_dim))

        self.dropout = nn.Dropout(p=dropout_rate)
        self.relu = nn.ReLU()
        self._graphs = _GraphCache()

    def forward(self, data):
        L.require_device(data.x, data.edge_index, *self.parameters(), what="MLP input")
        n_nodes = data.x.shape[0]
        x = _with_mask_input(data, self.with_mask).float()
        if x.numel() % self.input_dim != 0:
            raise RuntimeError(f"MLP: {x.numel()} input values are not rows of input_dim = {self.input_dim}")
        x = x.reshape(-1, self.input_dim)
        with torch.cuda.device(x.device):
            graph = self._graphs.get(data.edge_index, n_nodes, 0)      # only a handle: a K = 0 TAGConv runs no hop
            try:
                for layer in self.layers[:-1]:
                    x = self.relu(_hip_linear(graph, x, layer))
                    x = self.dropout(x)
                x = _hip_linear(graph, x, self.layers[-1])
            except RuntimeError as err:
                raise RuntimeError(f"MLP: the HIP GEMM entry point rejected a Linear of this model (input_dim {self.input_dim}, "
                                   f"hidden_dim {self.hidden_dim}, output_dim {self.output_dim}): {err}") from err
        return x.reshape(n_nodes, -1)
