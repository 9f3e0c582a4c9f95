"""Alchemical_NLL.potential_grad / .per_molecule_grad on the GPU: the values of
potential / per_molecule with a grad_fn that takes a per-molecule upstream
gradient (enflow_alchemical_nll_mol_backward_f32).

Reference: the float64 torch restatement of enflow/flow/loss.py per molecule
(tests/_energy_grad.py, pinned to the reference's goldens by
tests/test_energy_grad_host.py), and the goldens themselves on their batch.
Bars (the project's): values 1e-5 per element relative to the sum of the
absolute values of the element's terms, gradients 5e-5 normwise per tensor.
For every batch EG.reference first asserts that the float32 restatement stays
within half of each bar.  The upstream gradient is a fixed random [M] vector
with a zero and a negative entry (EG.upstreams; two of them for a batch of two
molecules, so that each molecule is weighted once).

Measured on one MI355X (worst over the cases of this file): see DESIGN 4.8.
"""
import numpy as np
import pytest
import torch

import _energy_grad as EG
import _reverse_grad as RG
from _fixtures import assert_all_within, load, normwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _nll(softening, kbt=None):
    from enflow_amd.flow import Alchemical_NLL
    return Alchemical_NLL(kBT=EG.kBT() if kbt is None else kbt, partition_func=EG.PF, softening=softening)


def _data(b, dtype=torch.float32, leaves=True):
    from enflow_amd.data import Data
    d = Data.from_arrays(b, device=DEV, dtype=dtype)
    if leaves:
        for k in EG.KEYS:
            getattr(d, k).requires_grad_(True)
    return d


def _run(b, softening, w, ldj, dtype=torch.float32, kbt=None):
    """Both calls with their backward: dict(pot, nll, gpot, gnll) as numpy
    (gradients: dict over h / g / pos / vel / ldj, None where autograd gave none)."""
    nll = _nll(softening, kbt)
    wt = torch.tensor(w, dtype=dtype, device=DEV)
    out = {}
    d = _data(b, dtype)
    pot = nll.potential_grad(d)
    (pot * wt).sum().backward()
    out["pot"], out["pot_t"] = pot.detach().cpu().numpy(), pot
    out["gpot"] = {k: getattr(d, k).grad for k in EG.KEYS}
    d = _data(b, dtype)
    lt = torch.tensor(ldj, dtype=dtype, device=DEV, requires_grad=True)
    val = nll.per_molecule_grad(d, lt)
    (val * wt).sum().backward()
    out["nll"], out["nll_t"] = val.detach().cpu().numpy(), val
    out["gnll"] = {k: getattr(d, k).grad for k in EG.KEYS}
    out["gnll"]["ldj"] = lt.grad
    torch.cuda.synchronize()
    return out


def _np(g):
    return {k: v.cpu().numpy() for k, v in g.items() if v is not None}


def _check(name, b, softening, r, got):
    M = len(b["mol_ptr"]) - 1
    assert got["pot"].shape == (M,) and got["nll"].shape == (M,)
    ev = {"pot": EG.value_errs(got["pot"], r["pot"], r["potS"]), "nll": EG.value_errs(got["nll"], r["nll"], r["nllS"])}
    # the energy depends on pos alone
    assert all(got["gpot"][k] is None for k in ("h", "g", "vel")), "potential_grad gave h / g / vel a gradient"
    gpot, gnll = _np(got["gpot"]), _np(got["gnll"])
    assert set(gnll) == {"h", "g", "pos", "vel", "ldj"}
    eg = {f"pot.{k}": v for k, v in EG.grad_errs(gpot, {"pos": r["gpot"]["pos"]}).items()}
    eg.update({f"nll.{k}": v for k, v in EG.grad_errs(gnll, r["gnll"]).items()})
    print(f"{name} softening {softening}: values / S {ev}, worst gradient {max(eg.values()):.2e} "
          f"({max(eg, key=eg.get)}); float32 floor: values {r['floor']}, gradients {max(r['gfloor'].values()):.2e}")
    assert_all_within(ev, EG.VAL_TOL, f"{name}: values")
    assert_all_within(eg, EG.GRAD_TOL, f"{name}: gradients")
    assert np.array_equal(gnll["ldj"], -r["w"].astype(gnll["ldj"].dtype))
    # a molecule whose weight is zero gets exactly zero rows
    for m in np.flatnonzero(r["w"] == 0):
        s = slice(int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1]))
        assert not np.any(gpot["pos"][s]) and all(not np.any(gnll[k][s]) for k in EG.KEYS)


CASES = [(n, s) for n in ("n32", "n64", "n256", "lj", "nf12") for s in EG.GPU_BATCHES[n][4]]


@pytest.mark.parametrize("name,softening", CASES)
def test_values_and_gradients(name, softening):
    """n32: sizes [1, 2, 5, 22, 32] (a molecule with no pair, the last size of
    the <= 32 image), softening 0.1 and 0 (the unsoftened r^-14); n64 / n256: the
    64- and 256-atom images, a ragged batch; lj: LJ boxes [300, 7], the
    wave-per-atom path with a small molecule on it; nf12: the 16-feature library."""
    b, refs = EG.references(name, softening)
    for r in refs:
        got = _run(b, softening, r["w"], r["ldj"])
        assert got["pot"].dtype == np.float32 and got["nll"].dtype == np.float32
        _check(name, b, softening, r, got)


@pytest.mark.parametrize("name", ["coincident32", "coincident_lj"])
@pytest.mark.parametrize("softening", [0.0, 0.1])
def test_coincident_atoms_are_dropped(name, softening):
    """Two atoms in one place, in a <= 32-atom batch and in a > 256-atom one: the
    d^2 == 0 pair is dropped (with softening 0 it would be 1 / 0), and a
    two-atom molecule whose atoms coincide gets exactly zero force."""
    b, refs = EG.references(name, softening)
    m = {"coincident32": 0, "coincident_lj": 1}[name]              # the two-atom molecule
    s = slice(int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1]))
    assert s.stop - s.start == 2 and np.array_equal(b["pos"][s][0], b["pos"][s][1])
    assert any(r["w"][m] != 0 for r in refs)
    for r in refs:
        got = _run(b, softening, r["w"], r["ldj"])
        _check(name, b, softening, r, got)
        assert got["pot"][m] == 0.0
        assert not np.any(got["gpot"]["pos"].cpu().numpy()[s]) and not np.any(got["gnll"]["pos"].cpu().numpy()[s])


@pytest.mark.parametrize("name,softening", [("energy_grad_s01", 0.1), ("energy_grad_s0", 0.0)])
def test_against_the_reference_goldens(name, softening):
    """The goldens' batch (1, 2, 5, 22 atoms and a 5-atom molecule with a
    coincident pair), unit upstream: values and gradients against the
    reference's own float64 numbers."""
    inp, out = load(name)
    b = {k: inp[k].astype(np.float64) for k in EG.FLOATS}
    b["mol_ptr"] = inp["mol_ptr"].astype(np.int64)
    M = len(b["mol_ptr"]) - 1
    ldj, kbt = inp["ldj"].astype(np.float64), float(inp["kBT"])
    got = _run(b, softening, np.ones(M), ldj, kbt=kbt)
    potS, nllS = EG.scales(b, ldj, kbt, softening, float(inp["partition_func"]))
    ev = {"pot": EG.value_errs(got["pot"], out["pot"], potS), "nll": EG.value_errs(got["nll"], out["nll"], nllS)}
    gnll = _np(got["gnll"])
    eg = {"pot.pos": normwise(got["gpot"]["pos"].cpu().numpy(), out["dpot_pos"])}
    eg.update({f"nll.{k}": normwise(gnll[k], out[f"dnll_{k}"]) for k in EG.KEYS})
    print(f"{name}: values / S {ev}, gradients {eg}")
    assert_all_within(ev, EG.VAL_TOL, f"{name}: values")
    assert_all_within(eg, EG.GRAD_TOL, f"{name}: gradients")


def test_float64_inputs_come_back_float64():
    b = EG.gpu_batch("n32")
    r = EG.reference(b, "n32", 0.1, 0)
    got = _run(b, 0.1, r["w"], r["ldj"], dtype=torch.float64)
    assert got["pot"].dtype == np.float64 and got["nll"].dtype == np.float64
    assert got["gpot"]["pos"].dtype == torch.float64
    assert all(v.dtype == torch.float64 for v in got["gnll"].values())
    _check("n32 float64", b, 0.1, r, got)


@pytest.mark.parametrize("name", ["n32", "n256", "lj"])
def test_values_are_bitwise_the_inference_calls(name):
    b = EG.gpu_batch(name)
    r = EG.reference(b, name, 0.1, 0)
    nll = _nll(0.1)
    lt = torch.tensor(r["ldj"], dtype=torch.float32, device=DEV)
    with torch.no_grad():
        d = _data(b, leaves=False)
        pot0, val0 = nll.potential(d), nll.per_molecule(d, lt)
        assert torch.equal(nll.potential_grad(d), pot0) and torch.equal(nll.per_molecule_grad(d, lt), val0)
    d = _data(b, leaves=False)                                      # grad enabled, nothing requires a gradient
    p, v = nll.potential_grad(d), nll.per_molecule_grad(d, lt)
    assert torch.equal(p, pot0) and torch.equal(v, val0) and p.grad_fn is None and v.grad_fn is None
    d = _data(b)
    p, v = nll.potential_grad(d), nll.per_molecule_grad(d, lt.clone().requires_grad_(True))
    assert p.grad_fn is not None and v.grad_fn is not None
    assert torch.equal(p.detach(), pot0) and torch.equal(v.detach(), val0)
    # only ldj_mol requires a gradient
    d = _data(b, leaves=False)
    l2 = lt.clone().requires_grad_(True)
    v = nll.per_molecule_grad(d, l2)
    v.sum().backward()
    assert torch.equal(v.detach(), val0) and torch.equal(l2.grad, -torch.ones_like(l2))


@pytest.mark.parametrize("name", ["n32", "n256", "lj"])
def test_backward_is_bitwise_reproducible_and_zero_upstream_is_zero(name):
    b = EG.gpu_batch(name)
    r = EG.reference(b, name, 0.1, 0)
    g1 = _run(b, 0.1, r["w"], r["ldj"])
    g2 = _run(b, 0.1, r["w"], r["ldj"])
    assert torch.equal(g1["gpot"]["pos"], g2["gpot"]["pos"])
    assert all(torch.equal(g1["gnll"][k], g2["gnll"][k]) for k in g1["gnll"])
    z = _run(b, 0.1, np.zeros_like(r["w"]), r["ldj"])
    assert not torch.any(z["gpot"]["pos"]) and all(not torch.any(v) for v in z["gnll"].values())


def test_second_differentiation_raises():
    b = EG.gpu_batch("n32")
    nll = _nll(0.1)
    for call in (lambda d: nll.potential_grad(d), lambda d: nll.per_molecule_grad(d, torch.zeros(5, device=DEV))):
        d = _data(b)
        wt = torch.ones(5, device=DEV, requires_grad=True)         # an upstream gradient with history of its own
        (g,) = torch.autograd.grad((call(d) * wt).sum(), d.pos, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()


@pytest.mark.parametrize("name", ["n32", "n64", "lj"])
def test_cross_check_against_the_scalar_kernel(name):
    """per_molecule_grad(out, ldj_mol).mean() and the existing differentiable
    nll(out, ldj_mol.sum()) differ by a constant: their gradients agree to 1e-6
    normwise (only the summation order differs), and d / d ldj_mol is -1 / M."""
    b = EG.gpu_batch(name)
    r = EG.reference(b, name, 0.1, 0)
    nll = _nll(0.1)
    M = len(r["w"])
    d1, d2 = _data(b), _data(b)
    l1 = torch.tensor(r["ldj"], dtype=torch.float32, device=DEV, requires_grad=True)
    l2 = l1.detach().clone().requires_grad_(True)
    nll.per_molecule_grad(d1, l1).mean().backward()
    nll(d2, l2.sum()).backward()
    errs = {k: normwise(getattr(d1, k).grad.cpu().numpy(), getattr(d2, k).grad.cpu().numpy()) for k in EG.KEYS}
    print(f"{name}: per-molecule mean vs the batch scalar's backward: {errs}")
    assert_all_within(errs, 1e-6, f"{name}: against nll_bwd_kernel")
    assert torch.equal(l1.grad, torch.full_like(l1, -1.0 / M))
    assert normwise(l2.grad.cpu().numpy(), l1.grad.cpu().numpy()) <= 1e-6


# ---------------------------------------------------------------------------
# composition with LFIntegrator.reverse_grad: training by energy
# ---------------------------------------------------------------------------
_COMP = {}


def _composition():
    """The 2-layer, H 32 flow without dequantiser on 5 + 9 + 22 atoms and its
    float64 restatement (computed once)."""
    if not _COMP:
        from enflow_amd.data.synthetic import make_molecules, default_dt
        from enflow_amd.nn import EGCL
        from enflow_amd.flow import LFIntegrator
        b = make_molecules(3, [5, 9, 22], nf=5, seed=12)
        b["h"] = b["h"] + 0.3 * np.random.default_rng(1012).normal(size=b["h"].shape)
        for k in EG.FLOATS:
            b[k] = EG.f32(b[k])
        torch.manual_seed(11)
        model = LFIntegrator([EGCL(5, 5, 32) for _ in range(2)], None, dt=default_dt())
        _COMP.update(b=b, model=model, layers=RG.model_layers(model))
    return _COMP["b"], _COMP["model"], _COMP["layers"]


def _lj_mols(pos, mol_ptr, softening):
    return torch.stack([EG.lj_torch(pos[int(mol_ptr[m]):int(mol_ptr[m + 1])], softening)
                        for m in range(len(mol_ptr) - 1)])


def _energy_loss(U, ldj, kbt, weighted):
    per = U / kbt - ldj
    if weighted:     # importance weights of the generated samples, detached
        return (torch.softmax((-U / kbt + ldj).detach(), 0) * per).sum()
    return per.mean()


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "importance-weighted"])
def test_energy_training_step_composes_with_reverse_grad(weighted):
    """x, rev_ldj = flow.reverse_grad(z); loss = (potential_grad(x) / kBT -
    rev_ldj).mean(), or each molecule weighted by a detached softmax(-U / kBT +
    rev_ldj): loss to 1e-5, every parameter and input gradient to 5e-5 of the
    float64 restatement with the float64 LJ on top."""
    from enflow_amd.data import Data
    b, model, layers = _composition()
    soft, kbt = 0.5, EG.kBT()
    ref = {}
    for dtype in (torch.float64, torch.float32):
        out, P, leaves = RG.restate(layers, b, float(model.dt), dtype=dtype)
        loss = _energy_loss(_lj_mols(out["pos"], b["mol_ptr"], soft), out["ldj"], kbt, weighted)
        gl, gi = RG.grads_of(loss, P, leaves)
        ref[dtype] = (float(loss.detach()), {**{f"p{i}.{k}": v for i, p in enumerate(gl) for k, v in p.items()},
                                    **{f"in.{k}": v for k, v in gi.items()}})
    l64, g64 = ref[torch.float64]
    l32, g32 = ref[torch.float32]
    assert abs(l32 - l64) <= EG.VAL_TOL / 2 * abs(l64), "the float32 floor of the loss exceeds half the bar"
    assert_all_within({k: normwise(g32[k], g64[k]) for k in g64 if np.linalg.norm(g64[k]) > 0}, EG.GRAD_TOL / 2,
                      "float32 restatement of the energy gradients")
    model.to(DEV)
    model.zero_grad(set_to_none=True)
    d = Data.from_arrays(b, device=DEV)
    zin = {k: getattr(d, k).requires_grad_(True) for k in RG.KEYS}
    x, rev_ldj = model.reverse_grad(d)
    loss = _energy_loss(_nll(soft).potential_grad(x), rev_ldj, kbt, weighted)
    loss.backward()
    got = {f"in.{k}": v.grad.cpu().numpy() for k, v in zin.items()}
    for i, n in enumerate(model.networks):
        got.update({f"p{i}.{k}": p.grad.cpu().numpy() for k, p in n.named_parameters()})
    errs = {k: normwise(got[k], g64[k]) for k in g64 if np.linalg.norm(g64[k]) > 0}
    print(f"energy step ({'weighted' if weighted else 'mean'}): loss {loss.item():.6f} (float64 {l64:.6f}), worst "
          f"gradient err {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert abs(loss.item() - l64) <= EG.VAL_TOL * abs(l64)
    assert set(g64) <= set(got)
    assert_all_within(errs, EG.GRAD_TOL, "energy-step gradients")
