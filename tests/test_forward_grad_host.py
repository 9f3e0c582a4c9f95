"""CPU checks behind LFIntegrator.forward_grad: the one-molecule-at-a-time
reference of tests/_forward_grad.py against the whole-batch gradient oracle
(values and every gradient), and the new surface (CPU tensors and node_nf 17
refused, the expansion entry exported, bound and validating its arguments).

Reference: enflow/flow/dynamics.py:10-24, enflow/nn/argmax.py:13-25.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle.enflow_oracle_grad import flow_forward_torch, train_loss_and_grads, _nll
from _fixtures import normwise, scalar_rel, assert_all_within
import _forward_grad as FG

NAME = "enflow_ldj_mol_to_atoms_f32"
KBT, SOFT, PF = 0.6, 0.1, 10.0


def _case(kind, seed):
    from enflow_amd.nn import EGCL, ArgMax, Floor
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import make_molecules, default_dt
    b = make_molecules(3, [3, 4, 22], nf=5, seed=seed)
    torch.manual_seed(seed + 1)
    nets = [EGCL(5, 5, 32), EGCL(5, 5, 32, attention=True, tanh=True)]
    dq = ArgMax(5, 32) if kind == "argmax" else Floor(dequant_scale=0.9)
    model = LFIntegrator(nets, dq, dt=default_dt())
    rng = np.random.default_rng(seed + 2)
    eps = rng.normal(size=b["h"].shape) if kind == "argmax" else rng.uniform(size=b["h"].shape)
    return FG.model_parts(model) + (b, eps, float(model.dt))


@pytest.mark.parametrize("kind,seed", [("argmax", 11), ("floor", 21)])
def test_per_molecule_values_sum_to_the_batch_scalar(kind, seed):
    layers, dq, k, b, eps, dt = _case(kind, seed)
    assert k == kind
    M = len(b["mol_ptr"]) - 1
    ref = FG.reference(layers, dq, b, eps, dt, kind, np.ones(M), {})
    with torch.no_grad():
        h, g, pos, vel, ldj, *_ = flow_forward_torch(layers, dq, b, eps, dt, 1.0, kind)
    whole = dict(h=h, g=g, pos=pos, vel=vel)
    errs = {k_: normwise(ref["out"][k_], whole[k_].numpy()) for k_ in FG.KEYS}
    errs["ldj"] = scalar_rel(float(np.sum(ref["ldj_mol"])), float(ldj))
    print(kind, errs, "constant share", FG.constant_share(kind, M))
    assert (FG.constant_share(kind, M) != 0) == (kind == "argmax")
    assert_all_within(errs, 1e-12, "one molecule at a time vs the whole batch")


@pytest.mark.parametrize("kind,seed", [("argmax", 11), ("floor", 21)])
def test_per_molecule_gradients_reproduce_the_training_step(kind, seed):
    """The training loss is the weighted sum it is: w = -1 / M on every ldj_mol,
    the NLL's output terms as cotangents (autograd of the NLL on the helper's
    outputs as leaves)."""
    layers, dq, _, b, eps, dt = _case(kind, seed)
    M = len(b["mol_ptr"]) - 1
    loss, ldj, gl, gd, out, gi = train_loss_and_grads(layers, dq, b, eps, dt, KBT, SOFT, PF, dequant_kind=kind,
                                                      input_grads=True)
    vals = FG.reference(layers, dq, b, eps, dt, kind, np.zeros(M), {})["out"]
    leaves = {k: torch.tensor(vals[k]).requires_grad_(True) for k in FG.KEYS}
    _nll(leaves["h"], leaves["g"], leaves["pos"], leaves["vel"], torch.tensor(0.0, dtype=torch.float64),
         np.asarray(b["mol_ptr"], dtype=np.int64), KBT, SOFT, PF).backward()
    c = {k: v.grad.numpy() for k, v in leaves.items()}
    ref = FG.reference(layers, dq, b, eps, dt, kind, np.full(M, -1.0 / M), c)
    errs = {f"in.{k}": normwise(ref["gi"][k], gi[k]) for k in gi}
    assert set(gi) == set(ref["gi"]) and ("h" in gi) == (kind == "floor")
    for i, (a, r) in enumerate(zip(ref["gl"], gl)):
        errs.update({f"p{i}.{k}": normwise(a[k], r[k]) for k in r})
    errs.update({f"dq.{k}": normwise(ref["gd"][k], gd[k]) for k in gd})
    assert (len(gd) > 0) == (kind == "argmax")
    assert all(np.linalg.norm(v) > 0 for v in gi.values())
    print(kind, "worst", max(errs.values()), max(errs, key=errs.get))
    assert_all_within(errs, 1e-12, "per-molecule construction vs train_loss_and_grads")


def test_upstream_has_a_zero_a_negative_and_distinct_entries():
    for M in (2, 3, 5):
        w = FG.upstream(M)
        assert np.sum(w == 0) == 1 and np.sum(w < 0) == 1 and len(set(w.tolist())) == M
        assert np.array_equal(w, w.astype(np.float32).astype(np.float64))


def _cpu_flow(nf=5):
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data import Data
    from enflow_amd.data.synthetic import make_molecules, default_dt
    torch.manual_seed(0)
    model = LFIntegrator([EGCL(nf, nf, 32) for _ in range(2)], ArgMax(nf, 32), dt=default_dt())
    return model, Data.from_arrays(make_molecules(2, [3, 4], nf=nf, seed=0), device="cpu")


def test_forward_grad_refuses_cpu_tensors_and_wide_features():
    from enflow_amd import _lib
    model, d = _cpu_flow()
    with pytest.raises(_lib.HipPathError):          # the training branch
        model.forward_grad(d)
    with torch.no_grad():                           # forward(per_molecule=True)
        with pytest.raises(_lib.HipPathError):
            model.forward_grad(d)
    # forward(per_molecule=True) under autograd stays refused and names both ways out
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*forward_grad"):
        model.forward(d, per_molecule=True)
    wide, dw = _cpu_flow(nf=17)
    with pytest.raises(NotImplementedError):
        wide.forward_grad(dw)


@pytest.mark.parametrize("nf", [None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_entry_exported_bound_and_refuses_bad_arguments(nf):
    from enflow_amd import _lib
    L = _lib.lib(nf)
    assert L.enflow_abi_version() == 13              # additive
    assert hasattr(L, NAME) and NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    fn = getattr(L, NAME)
    assert fn.restype is res and list(fn.argtypes) == list(args)
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "enflow_hip.h")).read()
    assert NAME in hdr and "#define ENFLOW_BWD_LDJ_ATOMS 0x800" in hdr
    assert _lib.BWD_LDJ_ATOMS == 0x800 and not _lib.BWD_LDJ_ATOMS & (_lib.BWD_F32 | _lib.EGCL_VARIANTS | 0xff)
    buf = ctypes.create_string_buffer(64)            # never dereferenced: every call is refused or has nothing to do
    P = ctypes.addressof(buf)
    assert fn(-1, 4, P, P, P, None) == -1 and fn(1, -1, P, P, P, None) == -1
    for i in (2, 3, 4):
        a = [1, 4, P, P, P, None]
        a[i] = None
        assert fn(*a) == -1, i
    assert fn(0, 0, None, None, None, None) == 0 and fn(2, 0, P, P, P, None) == 0
