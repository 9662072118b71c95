"""Float64 restatement of the baselines (plain torch, CPU): PyG's published `gcn_norm` / `add_remaining_self_loops` and
`GCNConv.forward`, the reference's GCN and MLP classes (networks/GCN.py, networks/MLP.py) and its Tikhonov formula
(collaborative_filtering.py:75-79).  PyG is not installed where the tests run, so tests/test_baselines_host.py pins the semantics of
`gcn_conv64` with closed forms, independently of this restatement."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def gated_relu(z, gate=None, record=None):
    """relu(z), or "z where gate else 0" with decisions imposed from outside (the idiom of oracle/ref_cpu.gated_relu); `record`
    receives this call's own ~(z <= 0)."""
    if record is not None:
        record.append((~(z <= 0)).detach())
    return F.relu(z) if gate is None else torch.where(gate.to(torch.bool), z, torch.zeros((), dtype=z.dtype))


def gcn_norm64(edge_index, n):
    """torch_geometric.nn.conv.gcn_conv.gcn_norm with edge_weight=None, add_self_loops=True, flow source_to_target:
    add_remaining_self_loops (stored self edges go, every node gets one loop of weight 1), deg = scatter_add of the weights over
    the TARGET index, weight_e = deg^-1/2[src] * deg^-1/2[dst] (inf -> 0).  Returns (src, dst, weight) with the loops appended."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    keep = src != dst
    loop = torch.arange(n, dtype=torch.long)
    src, dst = torch.cat([src[keep], loop]), torch.cat([dst[keep], loop])
    w = torch.ones(src.shape[0], dtype=torch.float64)
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, w)
    dis = deg.pow(-0.5)
    dis = torch.where(torch.isinf(dis), torch.zeros_like(dis), dis)
    return src, dst, dis[src] * w * dis[dst]


def gcn_degrees(edge_index, n):
    """d_i = 1 + #{stored e: dst(e) = i, src(e) != i} (int64)."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    keep = src != dst
    return torch.ones(n, dtype=torch.long).index_add_(0, dst[keep], torch.ones(int(keep.sum()), dtype=torch.long))


def gcn_conv64(x, edge_index, weight, bias=None):
    """GCNConv.forward: x = lin(x); out = propagate(aggr='add') of norm_e * x_src onto dst; out += bias.  float64."""
    x, weight = x.double(), weight.double()
    h = x @ weight.t()
    src, dst, w = gcn_norm64(edge_index, x.shape[0])
    out = torch.zeros_like(h).index_add_(0, dst, h[src] * w[:, None])
    return out if bias is None else out + bias.double()


class _Conv64(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.lin = nn.Linear(cin, cout, bias=False).double()
        self.bias = nn.Parameter(torch.zeros(cout, dtype=torch.float64))

    def forward(self, x, edge_index):
        return gcn_conv64(x, edge_index, self.lin.weight, self.bias)


class GCN64(nn.Module):
    """networks/GCN.py:5-21 in float64, same state_dict keys.  `gates`: None, or the two hidden layers' decisions ([N, hidden],
    nonzero = on) to impose; `recorded_gates` holds the last forward's own."""

    def __init__(self, nfeature_dim, output_dim, hidden_dim, with_mask=False):
        super().__init__()
        self.with_mask = with_mask
        self.conv1, self.conv2, self.conv3 = _Conv64(nfeature_dim, hidden_dim), _Conv64(hidden_dim, hidden_dim), _Conv64(hidden_dim, output_dim)
        self.gates, self.recorded_gates = None, []

    def forward(self, data):
        x = data.x.double()
        if self.with_mask:
            x = torch.cat([x, data.pred_mask.double()], dim=1)
        rec = []
        g = self.gates or (None, None)
        x = gated_relu(self.conv1(x, data.edge_index), g[0], rec)
        x = gated_relu(self.conv2(x, data.edge_index), g[1], rec)
        self.recorded_gates = rec
        return self.conv3(x, data.edge_index)


class MLP64(nn.Module):
    """networks/MLP.py:4-30 in float64 (eval: no dropout), one output row per node; `pre` keeps the last forward's hidden
    pre-activations."""

    def __init__(self, input_dim, output_dim, hidden_dim, num_layers, with_mask=False):
        super().__init__()
        self.input_dim, self.with_mask = input_dim, with_mask
        dims = [input_dim] + [hidden_dim] * num_layers + [output_dim]
        self.layers = nn.ModuleList([nn.Linear(a, b).double() for a, b in zip(dims[:-1], dims[1:])])
        self.pre = []

    def forward(self, data):
        x = data.x.double()
        if self.with_mask:
            x = torch.cat([x, data.pred_mask.double()], dim=1)
        n = x.shape[0]
        x = x.reshape(-1, self.input_dim)
        self.pre = []
        for layer in self.layers[:-1]:
            z = layer(x)
            self.pre.append(z.detach())
            x = F.relu(z)
        return self.layers[-1](x).reshape(n, -1)


def laplacian64(edge_index, n):
    """numpy-style construction of D - A with A_ij = number of stored lines between i and j."""
    a = torch.zeros(n, n, dtype=torch.float64)
    for s, d in edge_index.t().tolist():
        a[s, d] += 1
        if s != d:
            a[d, s] += 1
    return torch.diag(a.sum(1)) - a


def tikhonov64(alpha, lap, y):
    """inv(alpha L + I) L y exactly as the reference writes it (an explicit inverse), float64."""
    lap = lap.double()
    return torch.linalg.inv(alpha * lap + torch.eye(lap.shape[0], dtype=torch.float64)) @ lap @ y.double()
