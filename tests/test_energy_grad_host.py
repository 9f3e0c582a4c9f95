"""CPU-only checks of the differentiable per-molecule energies
(Alchemical_NLL.potential_grad / .per_molecule_grad,
enflow_alchemical_nll_mol_backward_f32):

* the float64 torch restatement of enflow/flow/loss.py per molecule
  (tests/_energy_grad.py) reproduces the reference's goldens
  (tests/golden/energy_grad_*.npz, written by make_golden_energy.py) to 1e-12;
* the closed-form gradient the kernels implement (numpy, no autograd) matches
  that restatement's autograd to 1e-12, the d^2 == 0 mask and a one-atom
  molecule included;
* on every batch of tests/test_gpu_energy_grad.py the float32 restatement is
  within HALF of each GPU bar (values 1e-5 of the sum of absolute terms,
  gradients 5e-5 normwise), so those bars test the kernels, not the inputs;
* the Python surface: CPU tensors, a wrong ldj_mol length, the exported symbol.
"""
import numpy as np
import pytest
import torch

import _energy_grad as EG
from _fixtures import load, normwise
from enflow_amd import _lib

GOLDENS = [("energy_grad_s01", 0.1), ("energy_grad_s0", 0.0)]
NAME = "enflow_alchemical_nll_mol_backward_f32"


def _golden_batch(inp):
    b = {k: inp[k].astype(np.float64) for k in EG.FLOATS}
    b["mol_ptr"] = inp["mol_ptr"].astype(np.int64)
    return b


def _close(got, ref, tol=1e-12):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = max(float(np.max(np.abs(ref))) if ref.size else 0.0, 1.0)
    return float(np.max(np.abs(got - ref))) / scale <= tol if ref.size else True


@pytest.mark.parametrize("name,softening", GOLDENS)
def test_restatement_reproduces_the_reference_goldens(name, softening):
    inp, out = load(name)
    assert float(inp["softening"]) == softening
    assert list(np.diff(inp["mol_ptr"])) == [1, 2, 5, 22, 5]
    b = _golden_batch(inp)
    a0 = int(b["mol_ptr"][4])
    assert np.array_equal(b["pos"][a0 + 3], b["pos"][a0])            # the coincident pair
    M = len(b["mol_ptr"]) - 1
    ones = np.ones(M)
    pot, nll, leaves = EG.restate(b, inp["ldj"].astype(np.float64), float(inp["kBT"]), softening,
                                  float(inp["partition_func"]))
    assert _close(pot.detach().numpy(), out["pot"]) and _close(nll.detach().numpy(), out["nll"])
    assert out["pot"][0] == 0.0 and float(pot[0].detach()) == 0.0              # one atom: no pair
    gp, gn = EG.grads(pot, ones, leaves), EG.grads(nll, ones, leaves)
    assert _close(gp["pos"], out["dpot_pos"])
    for k in EG.KEYS:
        assert _close(gn[k], out[f"dnll_{k}"]), k
        if k != "pos":
            assert not np.any(gp[k]), k                               # the energy depends on pos alone
    assert np.array_equal(gn["ldj"], -ones)
    assert np.all(np.isfinite(out["dpot_pos"]))                       # softening 0: the d^2 == 0 pair is dropped


@pytest.mark.parametrize("name,softening", GOLDENS)
def test_closed_form_matches_the_goldens(name, softening):
    inp, out = load(name)
    b = _golden_batch(inp)
    ones = np.ones(len(b["mol_ptr"]) - 1)
    cpot, cnll = EG.coefs(float(inp["kBT"]))
    assert _close(EG.closed_form(b, ones, cpot, softening)["pos"], out["dpot_pos"])
    got = EG.closed_form(b, ones, cnll, softening)
    for k in EG.KEYS:
        assert _close(got[k], out[f"dnll_{k}"]), k


@pytest.mark.parametrize("name", list(EG.GPU_BATCHES))
def test_closed_form_matches_autograd_and_float32_floor(name):
    """Every batch of the GPU test: the closed form against the float64
    restatement's autograd (1e-12 normwise), and -- inside EG.reference -- the
    float32 restatement within half of each GPU bar."""
    for softening in EG.GPU_BATCHES[name][4]:
        b, refs = EG.references(name, softening)
        for r in refs:
            _closed_form_vs(name, softening, b, r)


def _closed_form_vs(name, softening, b, r):
    assert np.any(r["w"] == 0) and np.any(r["w"] < 0)
    cpot, cnll = EG.coefs(r["kBT"])
    for coef, ref in ((cpot, r["gpot"]), (cnll, r["gnll"])):
        got = EG.closed_form(b, r["w"], coef, softening)
        for k in EG.KEYS:
            if np.linalg.norm(ref[k]) == 0:
                assert not np.any(got[k]), (name, k)
            else:
                assert normwise(got[k], ref[k]) <= 1e-12, (name, softening, k, normwise(got[k], ref[k]))
    assert np.array_equal(r["gnll"]["ldj"], -r["w"])
    # a zero weight: exactly zero rows
    m = int(np.flatnonzero(r["w"] == 0)[0])
    s = slice(int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1]))
    assert not np.any(r["gnll"]["pos"][s]) and not np.any(r["gnll"]["h"][s])


def test_coincident_atoms_and_one_atom_molecule_give_zero_force():
    pos = np.array([[0.25, -0.5, 1.0]])
    assert not np.any(EG.lj_force(pos, 0.0)) and not np.any(EG.lj_force(pos, 0.1))
    two = np.repeat(pos, 2, axis=0)                                   # both atoms in one place
    for s in (0.0, 0.1):
        assert not np.any(EG.lj_force(two, s))
        t = torch.tensor(two, requires_grad=True)
        (g,) = torch.autograd.grad(EG.lj_torch(t, s) + 0 * t.sum(), t)
        assert not torch.any(g) and float(EG.lj_torch(t, s).detach()) == 0.0
    three = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.1, 0.2, -0.3]])
    f = EG.lj_force(three, 0.0)
    assert np.all(np.isfinite(f)) and np.array_equal(f[0], f[1]) and np.allclose(f[0] + f[1] + f[2], 0.0, atol=1e-12)


# ---------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------
def _cpu_data():
    from enflow_amd.data import Data
    from enflow_amd.data.synthetic import make_molecules
    return Data.from_arrays(make_molecules(2, [3, 4], seed=0), device="cpu")


def test_new_names_refuse_cpu_tensors():
    from enflow_amd.flow import Alchemical_NLL
    nll, d = Alchemical_NLL(kBT=1.0), _cpu_data()
    with pytest.raises(_lib.HipPathError):
        nll.potential_grad(d)
    with pytest.raises(_lib.HipPathError):
        nll.per_molecule_grad(d, torch.zeros(2))
    d.pos.requires_grad_(True)
    with pytest.raises(_lib.HipPathError):
        nll.potential_grad(d)
    with pytest.raises(_lib.HipPathError):
        nll.per_molecule_grad(d, torch.zeros(2, requires_grad=True))


def test_wrong_length_ldj_mol_raises_value_error(monkeypatch):
    from enflow_amd.flow import Alchemical_NLL
    monkeypatch.setattr(_lib, "require_gpu", lambda t: None)          # reach the length check on a CPU machine
    nll, d = Alchemical_NLL(kBT=1.0), _cpu_data()
    for grad in (False, True):
        d.pos.requires_grad_(grad)
        with pytest.raises(ValueError, match="3 elements, the batch 2 molecules"):
            nll.per_molecule_grad(d, torch.zeros(3))


def test_refusals_of_the_inference_calls_name_the_new_methods(monkeypatch):
    from enflow_amd.flow import Alchemical_NLL
    monkeypatch.setattr(_lib, "require_gpu", lambda t: None)
    nll, d = Alchemical_NLL(kBT=1.0), _cpu_data()
    d.pos.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*potential_grad"):
        nll.potential(d)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*per_molecule_grad"):
        nll.per_molecule(d, torch.zeros(2))


@pytest.mark.parametrize("nf", [None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_entry_exported_bound_and_refuses_bad_arguments(nf):
    import ctypes
    import os
    import re
    L = _lib.lib(nf)
    assert L.enflow_abi_version() == 13                               # additive
    assert hasattr(L, NAME) and NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    fn = getattr(L, NAME)
    assert fn.restype is res and list(fn.argtypes) == list(args)
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "enflow_hip.h")).read()
    proto = re.search(NAME + r"\(([^)]*)\)", hdr)
    assert proto and len(proto.group(1).split(",")) == len(args) == 17
    # never dereferenced: every call below is refused before a launch (or has nothing to launch)
    buf = ctypes.create_string_buffer(64)
    P = ctypes.addressof(buf)
    coef = (ctypes.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    good = [1, 5, 5, 5, P, None, None, P, None, 0.1, P, coef, None, None, P, None, None]
    for i in (4, 7, 10, 11, 14):                                      # mol_ptr, pos, grad_out, coef, adj_pos
        bad = list(good)
        bad[i] = None
        assert fn(*bad) == -1, i
    for i in (12, 13, 15):                                            # an adjoint without its input
        bad = list(good)
        bad[i] = P
        assert fn(*bad) == -1, i
    assert fn(*([-1] + good[1:])) == -1
    assert fn(*(good[:3] + [0] + good[4:])) == -1                     # node_nf
    assert fn(*([0] + good[1:])) == 0                                 # nothing to do
