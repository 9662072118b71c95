"""The yardstick of `pfn_contingency_model_batch` (csrc/contingency_model.hip): the batch that the dataset (datasets/PowerFlowData.py)
and its collate build for the graphs "scenario s without line k", in torch on the CPU.  The dataset's arithmetic in fp32, in its
order: y * (1 - mask), then (v - mean) / (std + 1e-7); the reduced lists by `_verify_removed`'s index rule, idx = ar + (ar >= k).
tests/test_contingency_model_host.py holds it to `PowerFlowData` itself, bit for bit."""
import torch

from poweflownet_amd.datasets import PowerFlowData


def chunk_items(item0, chunk, S, e):
    """the items of the chunk that starts at `item0`: consecutive, the tail repeating the last item"""
    return [min(item0 + b, S * e - 1) for b in range(chunk)]


def kept_lines(k, e):
    """the lines that stay when line k is out, in stored order"""
    ar = torch.arange(e - 1)
    return ar + (ar >= k)


def _stat(v, count):
    return None if v is None else torch.as_tensor(v, dtype=torch.float32).reshape(-1)[:count].reshape(1, count)


def normalise(v, mean, std):
    """the dataset's (v - mean) / (std + 1e-7) in fp32; None, None: v itself"""
    if mean is None and std is None:
        return v
    mean = torch.zeros(1, v.shape[-1]) if mean is None else mean
    divisor = torch.ones(1, v.shape[-1]) if std is None else std + 0.0000001
    return (v - mean) / divisor


def batch_ref(bus_type, spec, edge_index, rx, items, xymean=None, xystd=None, edgemean=None, edgestd=None):
    """dict of CPU tensors: x [B n, 4], pred_mask [B n, 4] float32, bus_type [B n] int64, edge_index [2, B (e - 1)] int64, edge_attr
    [B (e - 1), 2] float32, batch [B n], ptr [B + 1] for the items (s * e + k) of one chunk.  bus_type [n] integer, spec [S, n, 4] and
    rx [S, e, 2] float64, edge_index [2, e] int64, all on the CPU."""
    n, e, B = int(spec.shape[1]), int(edge_index.shape[1]), len(items)
    table = torch.tensor(PowerFlowData.bus_type_mask)
    bt = bus_type.to(torch.long)
    mask = table[bt].float()
    xm, xs, em, es = _stat(xymean, 4), _stat(xystd, 4), _stat(edgemean, 2), _stat(edgestd, 2)
    xs_, ms_, bts, srcs, dsts, eas = [], [], [], [], [], []
    for b, item in enumerate(items):
        s, k = divmod(int(item), e)
        y = spec[s].float()
        xs_.append(normalise(y * (1.0 - mask), xm, xs))
        ms_.append(mask)
        bts.append(bt)
        idx = kept_lines(k, e)
        srcs.append(edge_index[0, idx] + b * n)
        dsts.append(edge_index[1, idx] + b * n)
        eas.append(normalise(rx[s, idx].float(), em, es))
    return {"x": torch.cat(xs_), "pred_mask": torch.cat(ms_), "bus_type": torch.cat(bts),
            "edge_index": torch.stack([torch.cat(srcs), torch.cat(dsts)]), "edge_attr": torch.cat(eas),
            "batch": torch.arange(B).repeat_interleave(n), "ptr": torch.arange(B + 1) * n}


def merged_ref(out, bus_type, spec_rows, xymean=None, xystd=None):
    """the merged, de-normalised table [B, n, 4] float32 of a chunk: `denormalize(out)` -- out * (std + 1e-7) + mean, two roundings --
    where the bus type's mask says "predict", float(spec) where the entry is given.  `out` [B n, 4] and `spec_rows` [B, n, 4] (the
    scenario of every chunk position) on one device."""
    dev = out.device
    B, n = int(spec_rows.shape[0]), int(spec_rows.shape[1])
    mask = torch.tensor(PowerFlowData.bus_type_mask)[bus_type.to(torch.long).cpu()].to(dev).bool()       # [n, 4]
    sd = torch.ones(1, 4) if xystd is None else _stat(xystd, 4) + 0.0000001
    mu = torch.zeros(1, 4) if xymean is None else _stat(xymean, 4)
    pred = out.view(B, n, 4) * sd.to(dev)                                  # (identity: * 1 + 0 all the same, as the kernel: -0 becomes +0)
    pred = pred + mu.to(dev)
    return torch.where(mask[None], pred, spec_rows.float())
