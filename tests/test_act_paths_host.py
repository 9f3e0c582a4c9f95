"""CPU side of tests/test_gpu_act_paths.py: what makes the float64 oracles a
reference at the non-default activation parameters used there, and the premises
of its cases.

0.1 oracle.enflow_oracle.activation (numpy) and oracle.enflow_oracle_grad._activation
    (torch functional) against torch's modules in float64, on a grid that holds
    every branch point and its float64 neighbours (the oracle goldens never cross
    a branch); the derivative under autograd away from the kinks.
0.2 both sides of every branch hold at least 1 % of the pre-activations of the
    section 1 training step (a condition on the inputs; mish's z > 20 arm is out
    of reach at these scales and is pinned in 0.1 only).
0.3 the float32 oracle of the section 1 step is within half of each bar of the
    float64 one, for every kind (the GPU cases assert the same, case by case).
"""
import numpy as np
import pytest
import torch

from oracle import enflow_oracle as O
from oracle import enflow_oracle_grad as OG
from _fixtures import act_module
from test_gpu_act_paths import CODES, train_setup, train_ref, oracle_step

ALL = dict(CODES, silu=(0, 0, 0))


def _kinks(name):
    """Branch points of the kind's function (its derivative need not exist there)."""
    k, p0, p1 = CODES.get(name, (0, 0, 0))
    if name in ("relu", "leaky", "elu", "celu", "selu"):
        return [0.0]
    if name == "softplus":
        return [p1 / p0]
    if name == "hardtanh":
        return [float(p0), float(p1)]
    if name == "mish":
        return [20.0]
    return []


def _grid(name):
    """About 2,000 points over [-25, 25] with 0, every branch point and two float64 neighbours on each side."""
    pts = [np.linspace(-25.0, 25.0, 2001)]
    for c in [0.0] + _kinks(name):
        lo, hi = np.nextafter(c, -np.inf), np.nextafter(c, np.inf)
        pts.append(np.array([np.nextafter(lo, -np.inf), lo, c, hi, np.nextafter(hi, np.inf)]))
    return np.unique(np.concatenate(pts))


@pytest.mark.parametrize("name", list(ALL))
def test_oracle_activation_is_torchs_module(name):
    code = ALL[name]
    x = _grid(name)
    for c in _kinks(name):
        assert c in x and np.nextafter(c, np.inf) in x and np.nextafter(c, -np.inf) in x
    if name == "softplus":      # the grid has points on both sides of z * p0 > p1 next to the threshold
        near = x[np.abs(x - code[2] / code[1]) < 1e-15]
        assert np.any(near * code[1] > code[2]) and np.any(near * code[1] <= code[2])
    mod = act_module(code)
    want = mod(torch.tensor(x)).numpy()
    got = O.activation(code)(x)
    assert got.dtype == np.float64 and want.dtype == np.float64
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    tgot = OG._activation(code)(torch.tensor(x)).numpy()
    terr = np.abs(tgot - want) / np.maximum(1.0, np.abs(want))
    # derivative away from the kinks
    keep = ~np.isin(x, _kinks(name))
    xa = torch.tensor(x[keep], requires_grad=True)
    xb = torch.tensor(x[keep], requires_grad=True)
    da, = torch.autograd.grad(OG._activation(code)(xa).sum(), xa)
    db, = torch.autograd.grad(mod(xb).sum(), xb)
    derr = np.abs(da.numpy() - db.numpy()) / np.maximum(1.0, np.abs(db.numpy()))
    print(f"{name} {code}: {x.size} points, numpy oracle {err.max():.1e}, torch oracle {terr.max():.1e}, "
          f"derivative {derr.max():.1e}")
    assert err.max() <= 1e-12 and terr.max() <= 1e-12 and derr.max() <= 1e-12


def _sides(name, z):
    k, p0, p1 = CODES[name]
    if name in ("relu", "leaky", "elu", "celu", "selu"):
        return {"z <= 0": z <= 0, "z > 0": z > 0}
    if name == "softplus":
        return {"z * p0 <= p1": z * p0 <= p1, "z * p0 > p1": z * p0 > p1}
    if name == "hardtanh":
        return {"z < p0": z < p0, "p0 <= z <= p1": (z >= p0) & (z <= p1), "z > p1": z > p1}
    raise KeyError(name)


@pytest.mark.parametrize("name", ["relu", "leaky", "elu", "celu", "selu", "softplus", "hardtanh"])
def test_both_sides_of_every_branch_are_taken(name, monkeypatch):
    """The pre-activations of the float64 oracle's section 1 step, every call
    site of the layers and the ArgMax together."""
    seen = []
    orig = OG._activation

    def recording(code):
        f = orig(code)

        def act(x):
            seen.append(x.detach().double().numpy().reshape(-1))
            return f(x)
        return act

    monkeypatch.setattr(OG, "_activation", recording)
    oracle_step(train_setup(name, "fused"), torch.float64)
    # per layer: edge_nn twice, vel_scaling_nn, coord_nn, node_nn; the ArgMax once
    assert len(seen) == 2 * 5 + 1
    z = np.concatenate(seen)
    shares = {k: float(np.mean(m)) for k, m in _sides(name, z).items()}
    print(f"{name} {CODES[name]}: {z.size} pre-activations in [{z.min():.2f}, {z.max():.2f}], shares "
          + ", ".join(f"{k}: {100 * v:.1f} %" for k, v in shares.items()))
    assert abs(sum(shares.values()) - 1.0) < 1e-12
    assert min(shares.values()) >= 0.01, shares


@pytest.mark.parametrize("name", list(CODES))
def test_float32_floor_of_the_training_step(name):
    """train_ref asserts the floor (loss: LOSS_TOL / 2, every gradient: GRAD_TOL / 2)."""
    (loss, grads), floor = train_ref(name, "fused")
    assert np.isfinite(loss) and all(np.all(np.isfinite(v)) for v in grads.values())
    print(f"{name}: worst float32-oracle gradient floor {floor:.2e}")
