"""The float64 twin of the optimiser step: torch.optim.Adam(foreach=False) -- torch's single-tensor implementation, the arithmetic
csrc/adam_math.hpp restates -- on CPU tensors of the given dtype, constructed as the reference constructs its optimiser
(scene/gaussian_model.py:222: lr=0.0, eps=1e-15) and given the learning rates the package's schedules give.  Test infrastructure
only.  tests/test_optim_host.py ties it to the reference's own methods (tests/golden/optim.npz)."""
import torch
from torch import nn

from mpmavatar_amd import optim


def make(groups, dtype=torch.float64):
    """groups: [{"name", "lr", "params": {tensor name: array}, ...}] -> (optimizer, {tensor name: Parameter})"""
    leaves, out = {}, []
    for g in groups:
        ps = {k: nn.Parameter(torch.tensor(v, dtype=dtype)) for k, v in g["params"].items()}
        leaves.update(ps)
        out.append({**{k: v for k, v in g.items() if k != "params"}, "params": list(ps.values())})
    return torch.optim.Adam(out, lr=0.0, eps=1e-15, foreach=False), leaves


def step(opt, leaves, grads, iteration=None):
    """one step with grads {tensor name: array or None (no gradient)}; iteration: the schedules are applied first"""
    if iteration is not None:
        optim.update_learning_rate(opt, iteration)
    for k, p in leaves.items():
        g = grads.get(k)
        p.grad = None if g is None else torch.tensor(g, dtype=p.dtype)
    opt.step()


def result(opt, leaves):
    """-> {"p_" / "m_" / "v_" + tensor name: array}; a parameter without state has zero moments"""
    out = {}
    for k, p in leaves.items():
        st = opt.state.get(p, {})
        out["p_" + k] = p.detach().numpy().copy()
        out["m_" + k] = st["exp_avg"].numpy().copy() if st else torch.zeros_like(p).numpy()
        out["v_" + k] = st["exp_avg_sq"].numpy().copy() if st else torch.zeros_like(p).numpy()
    return out
