"""The non-learned baseline of the reference's perfomance_evaluator.py: the Tikhonov graph regulariser
(`collaborative_filtering.py:75-79`) and the graph Laplacian it is given (pygsp's `graphs.Graph(adjacency).L`,
perfomance_evaluator.py:138-153), in float64, as plain torch ops on the device the caller's tensors live on."""
from __future__ import annotations

import torch


def graph_laplacian(edge_index: torch.Tensor, n: int) -> torch.Tensor:
    """D - A, [n, n] float64 on `edge_index`'s device, symmetric, with A_ij = the number of stored lines between i and j (either
    direction; a stored self edge counts once on the diagonal of A and cancels in D - A): what pygsp's combinatorial
    `Graph(adjacency).L` gives for the reference's adjacency file."""
    src, dst = edge_index[0], edge_index[1]
    a = torch.zeros(n, n, dtype=torch.float64, device=edge_index.device)
    ones = torch.ones(src.shape[0], dtype=torch.float64, device=edge_index.device)
    a.index_put_((src, dst), ones, accumulate=True)
    off = src != dst
    a.index_put_((dst[off], src[off]), ones[off], accumulate=True)
    return torch.diag(a.sum(dim=1)) - a


def tikhonov_operator(alpha: float, lap: torch.Tensor) -> torch.Tensor:
    """inv(alpha L + I) L as ONE `torch.linalg.solve` (per topology): [n, n] float64."""
    lap = lap.double()
    eye = torch.eye(lap.shape[0], dtype=torch.float64, device=lap.device)
    return torch.linalg.solve(alpha * lap + eye, lap)


def tikhonov_regularizer(alpha: float, lap: torch.Tensor, y: torch.Tensor, operator: torch.Tensor = None) -> torch.Tensor:
    """The reference's formula exactly as written: z = inv(alpha L + I) L y, float64 on the device.  `y`: [n, f] or [S, n, f]
    (one product per sample).  `operator`: a `tikhonov_operator(alpha, lap)` kept by a caller with many samples of one topology."""
    op = tikhonov_operator(alpha, lap) if operator is None else operator
    return torch.matmul(op, y.double())
