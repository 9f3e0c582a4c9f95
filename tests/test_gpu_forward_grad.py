"""LFIntegrator.forward_grad on the GPU: the per-molecule log|detJ| and every
gradient of a loss that weights it per molecule, against the float64 gradient
oracle run one molecule at a time (tests/_forward_grad.py, proved against the
whole-batch oracle in tests/test_forward_grad_host.py).

The loss is <w, ldj_mol> + sum_k <c_k, out_k>: w a fixed random [num_mols]
vector with a zero and a negative entry, all distinct, c fixed random
cotangents on g, pos, vel (and h where it is differentiable).  Bars, against
float64: 1e-5 normwise per output tensor, |got - ref| <= 1e-5 S_m per ldj_mol
element (S_m: the sum of the absolute values of the terms the element sums, the
metric of tests/test_gpu_ldj_mol.py), 5e-5 normwise per gradient tensor.  Each
case first asserts on the CPU that the same reference in float32 is within
half of each bar of the float64 one (seeds chosen for that).
"""
import numpy as np
import pytest
import torch

from _fixtures import normwise, assert_all_within
import _forward_grad as FG
import _energy_grad as EG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GRAD_TOL = 5e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _batch(sizes, nf=5, seed=0):
    from enflow_amd.data.synthetic import make_molecules
    b = make_molecules(len(sizes), list(sizes), nf=nf, seed=seed)
    for k in ("h", "g", "pos", "vel", "box", "r_cut"):
        b[k] = FG.f32(b[k])
    return b


def _small_batch(sizes, seed, scale=1e-3):
    """tests/test_gpu_small.py's recipe: features and g at `scale`."""
    b = _batch(sizes, seed=seed)
    b["h"] = FG.f32(np.floor(np.random.default_rng(seed + 1).uniform(0, 3, size=b["h"].shape)) * scale)
    b["g"] = FG.f32(b["g"] * scale)
    return b


def _model(kind, hid=32, nf=5, seed=11, prec="f16x3", small=None, **egcl_kw):
    from enflow_amd.nn import EGCL, ArgMax, Floor
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    torch.manual_seed(seed)
    nets = [EGCL(nf, nf, hid, **egcl_kw) for _ in range(2)]
    if small is not None:       # layer 1's edge_nn.0 at `small`: edge_nn.2's operand is entirely below 2^-7
        with torch.no_grad():
            nets[1].edge_nn[0].weight.mul_(small)
            nets[1].edge_nn[0].bias.mul_(small)
    dq = ArgMax(nf, hid) if kind == "argmax" else Floor() if kind == "floor" else None
    model = LFIntegrator(nets, dq, dt=default_dt())
    model.gemm_precision = prec
    return model


# name -> (model, batch); seeds for which the float32 reference meets half the bars (_reference asserts it)
CASES = {
    "base": (lambda: _model("none"), lambda: _batch([5, 9, 22], seed=12)),
    "argmax": (lambda: _model("argmax", seed=21), lambda: _batch([3, 4, 22], seed=22)),
    "floor": (lambda: _model("floor", seed=21), lambda: _batch([3, 4, 22], seed=22)),
    "n40": (lambda: _model("argmax", seed=31), lambda: _batch([40, 22], seed=32)),
    "n70": (lambda: _model("argmax", seed=41), lambda: _batch([70, 22], seed=42)),
    "nf12": (lambda: _model("none", hid=64, nf=12, seed=51), lambda: _batch([5, 22], nf=12, seed=52)),
    "variants": (lambda: _model("none", hid=64, seed=61, attention=True, norm_diff=True, tanh=True),
                 lambda: _batch([9, 22], seed=62)),
    "f32": (lambda: _model("none", prec="f32"), lambda: _batch([5, 9, 22], seed=12)),
    "small": (lambda: _model("none", seed=71, small=1e-3), lambda: _small_batch([5, 9, 22], seed=72)),
}
_BUILT, _REF = {}, {}


def _build(name):
    """(model on the device, batch, noise [A, nf] float64 or None, kind); built once per case."""
    if name not in _BUILT:
        model, b = CASES[name][0](), CASES[name][1]()
        kind = FG.model_parts(model)[2]
        rng = np.random.default_rng(5)
        noise = None if kind == "none" else FG.f32(rng.normal(size=b["h"].shape) if kind == "argmax"
                                                   else rng.uniform(size=b["h"].shape))
        _BUILT[name] = (model.to(DEV), b, noise, kind)
    return _BUILT[name]


def _upstream(b, kind):
    M = len(b["mol_ptr"]) - 1
    names = ("g", "pos", "vel") + (() if kind == "argmax" else ("h",))
    return FG.upstream(M), FG.cotangents(b, names)


def _reference(name):
    """The float64 reference of a case (cached, never modified) after the float32 floor check."""
    if name not in _REF:
        model, b, noise, kind = _build(name)
        layers, dq, _ = FG.model_parts(model)
        w, c = _upstream(b, kind)
        dt = float(model.dt)
        r64 = FG.reference(layers, dq, b, noise, dt, kind, w, c)
        r32 = FG.reference(layers, dq, b, noise, dt, kind, w, c, dtype=torch.float32)
        S = FG.scales(layers, dq, b, noise, dt, kind)
        f64, f32 = FG.flat(r64), FG.flat(r32)
        errs = {k: normwise(f32[k], f64[k]) for k in f64 if np.linalg.norm(f64[k]) > 0}
        el = float(np.max(np.abs(f32["ldj_mol"] - f64["ldj_mol"]) / S))
        print(f"{name}: float32 reference vs float64: worst output {max(v for k, v in errs.items() if k.startswith('out.')):.2e}, "
              f"ldj_mol / S {el:.2e}, worst gradient {max(v for k, v in errs.items() if not k.startswith('out.')):.2e}")
        assert_all_within({k: v for k, v in errs.items() if k.startswith("out.") or k == "ldj_mol"}, TOL / 2,
                          f"{name}: float32 reference values")
        assert el <= TOL / 2, f"{name}: float32 reference ldj_mol / S {el:.2e}"
        assert_all_within({k: v for k, v in errs.items() if not (k.startswith("out.") or k == "ldj_mol")}, GRAD_TOL / 2,
                          f"{name}: float32 reference gradients")
        _REF[name] = (f64, S)
    return _REF[name]


def _data(b):
    from enflow_amd.data import Data
    return Data.from_arrays(b, device=DEV)


def _noise(noise):
    return None if noise is None else torch.tensor(noise, dtype=torch.float32, device=DEV)


def _run(model, b, noise, w, c, scalar_k=None):
    """forward_grad + backward of <w, ldj_mol> + <c, out> (scalar_k: the plain
    forward with scalar_k * ldj instead).  Returns (values dict, gradients dict
    with the reference's names)."""
    model.zero_grad(set_to_none=True)
    d = _data(b)
    zin = {k: getattr(d, k).requires_grad_(True) for k in FG.KEYS}
    if scalar_k is None:
        out, ldj = model.forward_grad(d, noise=_noise(noise))
        loss = (ldj * torch.tensor(w, dtype=torch.float32, device=DEV)).sum()
    else:
        out, ldj = model(d, noise=_noise(noise))
        loss = scalar_k * ldj
    for k, ck in c.items():
        loss = loss + (getattr(out, k) * torch.tensor(ck, dtype=torch.float32, device=DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    vals = {f"out.{k}": getattr(out, k).detach().cpu().numpy() for k in FG.KEYS}
    vals["ldj_mol"] = ldj.detach().cpu().numpy()
    g = {f"in.{k}": (torch.zeros_like(v) if v.grad is None else v.grad).cpu().numpy() for k, v in zin.items()}
    for i, n in enumerate(model.networks):
        g.update({f"p{i}.{k}": p.grad.cpu().numpy() for k, p in n.named_parameters() if p.grad is not None})
    if model.dequantize is not None:
        g.update({f"dq.{k}": p.grad.cpu().numpy() for k, p in model.dequantize.named_parameters() if p.grad is not None})
    return vals, g, (out, ldj)


def _compare(name, ref, S, vals, g):
    oerr = {k: normwise(vals[k], ref[k]) for k in ref if k.startswith("out.")}
    el = np.abs(vals["ldj_mol"].astype(np.float64) - ref["ldj_mol"]) / S
    gerr = {}
    for k, r in ref.items():
        if k.startswith("out.") or k == "ldj_mol":
            continue
        assert k in g, f"{name}: no gradient for {k}"
        if np.linalg.norm(r) == 0:
            assert not np.any(g[k]), f"{name}: {k} is exactly zero in the reference"
            continue
        gerr[k] = normwise(g[k], r)
    print(f"{name}: worst output err {max(oerr.values()):.2e}, ldj_mol normwise {normwise(vals['ldj_mol'], ref['ldj_mol']):.2e} "
          f"worst element / S {float(np.max(el)):.2e}, worst gradient err {max(gerr.values()):.2e} "
          f"({max(gerr, key=gerr.get)})")
    assert_all_within(oerr, TOL, f"{name}: outputs")
    assert np.all(np.isfinite(vals["ldj_mol"])) and normwise(vals["ldj_mol"], ref["ldj_mol"]) <= TOL
    assert np.all(el <= TOL), f"{name}: ldj_mol elements over {TOL:g} * S_m: {el}"
    assert_all_within(gerr, GRAD_TOL, f"{name}: gradients")


@pytest.mark.parametrize("name", ["base", "argmax", "floor", "n40", "n70", "nf12", "variants", "f32", "small"])
def test_values_and_gradients(name):
    """base: the fused <= 32-atom instance, d h returned; argmax: argmax_bwd_kernel
    with a per-molecule d log q and ArgMax's parameter gradients; floor: d h through
    the dequantiser; n40: the 33..64-atom instance (taped pair list); n70: the BIG
    row blocks and the chunked ArgMax backward, whose third 32-atom window holds
    atoms of both molecules; nf12: the 16-feature library; variants: the VAR
    instance; f32: the ENFLOW_BWD_F32 backward; small: operands at 1e-3, one fp32
    re-run of the step, then the fp32 backward."""
    from enflow_amd import _lib
    model, b, noise, kind = _build(name)
    ref, S = _reference(name)
    w, c = _upstream(b, kind)
    n0 = _lib.FP32_RERUNS[0]
    vals, g, (out, ldj) = _run(model, b, noise, w, c)
    reruns = _lib.FP32_RERUNS[0] - n0
    assert ldj.shape == (len(w),) and ldj.dtype == torch.float32 and ldj.requires_grad
    assert out.g.requires_grad and out.pos.requires_grad and out.vel.requires_grad and out.h.requires_grad
    if name == "small":
        print("small operands: fp32 re-runs", reruns)
    assert reruns == (1 if name == "small" else 0)
    if kind == "argmax":
        assert "in.h" not in ref and not np.any(g["in.h"])      # the categorical data gets no gradient
        assert all(f"dq.{k}" in g for k in ("network.0.weight", "network.2.bias"))
    _compare(name, ref, S, vals, g)


@pytest.mark.parametrize("name", ["base", "argmax", "n70"])
def test_values_against_the_inference_call_and_the_scalar(name):
    """ldj_mol under autograd vs forward(per_molecule=True) under no_grad on the
    same noise: bitwise up to 64 atoms (the tape is a runtime argument of the same
    fused instance); n70 within the per-element bar, because training past 64
    atoms runs the large-system kernels where inference runs the fused 256-atom
    instance.  Under no_grad forward_grad IS that call: bitwise everywhere.
    Its float64 sum vs the plain training forward's scalar: one fp32 rounding of
    the total and one per element for the constant's share, times two."""
    model, b, noise, kind = _build(name)
    _, S = _reference(name)
    with torch.no_grad():
        inf, ldj_inf = model(_data(b), noise=_noise(noise), per_molecule=True)
        same, ldj_same = model.forward_grad(_data(b), noise=_noise(noise))
    assert torch.equal(ldj_inf, ldj_same) and not ldj_same.requires_grad
    for k in FG.KEYS:
        assert torch.equal(getattr(inf, k), getattr(same, k)), k
    out, ldj_mol = model.forward_grad(_data(b), noise=_noise(noise))
    _, scalar = model(_data(b), noise=_noise(noise))
    assert ldj_mol.requires_grad and scalar.requires_grad
    got, want = ldj_mol.detach().cpu().double().numpy(), ldj_inf.cpu().double().numpy()
    el = np.abs(got - want) / S
    print(f"{name}: autograd vs inference ldj_mol: bitwise {np.array_equal(got, want)}, worst element / S {el.max():.2e}")
    assert np.all(el <= TOL)
    if name != "n70":
        assert np.array_equal(got, want)
    tot, sc = float(got.sum()), float(scalar.detach())
    bound = 2.0 ** -21 * float(np.abs(got).sum())
    print(f"{name}: sum of elements {tot!r} vs the training scalar {sc!r} (bound {bound:.3e})")
    assert abs(tot - sc) <= bound


@pytest.mark.parametrize("name", ["base", "argmax", "n70"])
def test_constant_upstream_is_the_scalar_path_bitwise(name):
    """k * ldj_mol.sum() + f(out) through forward_grad vs k * ldj + f(out) through
    forward: the per-atom adjoint holds k everywhere, the arithmetic is the scalar
    call's, every gradient is torch.equal."""
    model, b, noise, kind = _build(name)
    w, c = _upstream(b, kind)
    k = 0.75
    _, g1, _ = _run(model, b, noise, np.full(len(w), k), c)
    _, g2, _ = _run(model, b, noise, None, c, scalar_k=k)
    assert set(g1) == set(g2)
    diff = {n: normwise(g1[n], g2[n]) for n in g1 if np.any(g2[n])}
    print(f"{name}: constant vector vs scalar path, worst normwise difference {max(diff.values()):.2e}")
    assert all(np.array_equal(g1[n], g2[n]) for n in g1), {n: v for n, v in diff.items() if v}


@pytest.mark.parametrize("name", ["base", "argmax", "n70"])
def test_one_hot_upstream_reaches_one_molecule(name):
    """w one-hot on molecule k, no output cotangents: the input-gradient rows of
    every other molecule are exactly zero, molecule k's equal those of a batch
    holding molecule k alone (1e-6 normwise; k the largest molecule, so that the
    batch of one runs the kernels the batch ran)."""
    model, b, noise, kind = _build(name)
    ptr = [int(x) for x in b["mol_ptr"]]
    M = len(ptr) - 1
    k = int(np.argmax(np.diff(ptr)))
    w = np.zeros(M)
    w[k] = 1.0
    _, g, _ = _run(model, b, noise, w, {})
    s1, n1 = FG.one(b, k, noise)
    _, ga, _ = _run(model, s1, n1, np.ones(1), {})
    errs = {}
    for key in ("in.g", "in.pos", "in.vel") + (() if kind == "argmax" else ("in.h",)):
        rows = g[key]
        assert not np.any(rows[:ptr[k]]) and not np.any(rows[ptr[k + 1]:]), key
        if not np.any(ga[key]):     # two layers: log|detJ| = log q + Q(h) + Q(h') does not depend on vel
            assert key == "in.vel" and not np.any(rows), key
            continue
        errs[key] = normwise(rows[ptr[k]:ptr[k + 1]], ga[key])
    print(f"{name}: molecule {k} in the batch vs alone", errs)
    assert_all_within(errs, 1e-6, "one-hot upstream vs the molecule alone")


@pytest.mark.parametrize("name", ["base", "argmax", "n70"])
def test_backward_is_reproducible_and_zero_upstream_gives_zeros(name):
    model, b, noise, kind = _build(name)
    w, c = _upstream(b, kind)
    v1, g1, _ = _run(model, b, noise, w, c)
    v2, g2, _ = _run(model, b, noise, w, c)
    assert all(np.array_equal(v1[k], v2[k]) for k in v1)
    assert set(g1) == set(g2) and all(np.array_equal(g1[k], g2[k]) for k in g1)
    _, g0, _ = _run(model, b, noise, np.zeros(len(w)), {k: np.zeros_like(v) for k, v in c.items()})
    assert set(g0) == set(g1) and all(not np.any(v) for v in g0.values())


class _NoGradient(torch.autograd.Function):
    """A consumer of the five outputs that passes None upstream to every one of them."""

    @staticmethod
    def forward(ctx, *ts):
        ctx.n = len(ts)
        return ts[0].new_zeros(())

    @staticmethod
    def backward(ctx, g):
        return (None,) * ctx.n


def test_all_none_upstream_returns_without_launching(monkeypatch):
    """Every upstream gradient None: _FlowFunction.backward is entered, returns
    None for every input before it allocates or launches anything, and no
    parameter gets a gradient."""
    from enflow_amd.flow import _train
    model, b, noise, _ = _build("base")
    model.zero_grad(set_to_none=True)
    calls, work = [], []
    orig = _train._FlowFunction.backward

    def backward(ctx, *grads):
        res = orig(ctx, *grads)
        calls.append((grads, res))
        return res

    monkeypatch.setattr(_train._FlowFunction, "backward", staticmethod(backward))
    monkeypatch.setattr(_train, "_adj", lambda *a, **k: work.append("adj") or pytest.fail("the backward went on"))
    monkeypatch.setattr(_train, "_alloc_ws", lambda *a, **k: work.append("ws") or pytest.fail("the backward went on"))
    out, ldj = model.forward_grad(_data(b), noise=_noise(noise))
    _NoGradient.apply(out.h, out.g, out.pos, out.vel, ldj).backward()
    assert len(calls) == 1 and not work
    grads, res = calls[0]
    assert len(grads) == 5 and all(g is None for g in grads)
    assert len(res) == 6 + len(list(model.parameters())) and all(r is None for r in res)
    assert all(p.grad is None for p in model.parameters())


def test_weighted_likelihood_step_composed_with_per_molecule_grad():
    """(w * nll.per_molecule_grad(out, ldj_mol)).sum() with w a detached softmax
    over molecules, 5 + 9 + 22 atoms, ArgMax: the loss and every gradient against
    the helper composed with tests/_energy_grad.py's per-molecule NLL; with
    w = 1 / M the gradients are the plain nll(out, ldj) step's to 1e-6 normwise
    (the bar DESIGN.md 4.8 uses for the same comparison on the loss side)."""
    from enflow_amd.flow import Alchemical_NLL
    model = _model("argmax", seed=81).to(DEV)
    b = _batch([5, 9, 22], seed=82)
    M = 3
    noise = FG.f32(np.random.default_rng(83).normal(size=b["h"].shape))
    kbt, soft = EG.kBT(), 0.1
    nll = Alchemical_NLL(kBT=kbt, softening=soft)

    def step(weights, plain=False):
        model.zero_grad(set_to_none=True)
        d = _data(b)
        zin = {k: getattr(d, k).requires_grad_(True) for k in ("g", "pos", "vel")}
        if plain:
            out, ldj = model(d, noise=_noise(noise))
            loss, wt = nll(out, ldj), None
        else:
            out, ldj_mol = model.forward_grad(d, noise=_noise(noise))
            vals = nll.per_molecule_grad(out, ldj_mol)
            wt = torch.softmax(-vals.detach() / vals.detach().abs().max(), 0) if weights is None else weights
            loss = (wt * vals).sum()
        loss.backward()
        g = {f"in.{k}": v.grad.cpu().numpy() for k, v in zin.items()}
        for i, n in enumerate(model.networks):
            g.update({f"p{i}.{k}": p.grad.cpu().numpy() for k, p in n.named_parameters()})
        g.update({f"dq.{k}": p.grad.cpu().numpy() for k, p in model.dequantize.named_parameters() if p.grad is not None})
        return float(loss), g, wt

    loss, g, wt = step(None)
    w = wt.cpu().double().numpy()
    assert abs(w.sum() - 1) < 1e-6 and len(set(w.tolist())) == M
    layers, dq, kind = FG.model_parts(model)
    dt = float(model.dt)

    def reference(dtype):
        r0 = FG.reference(layers, dq, b, noise, dt, kind, np.zeros(M), {}, dtype=dtype)
        st = dict(r0["out"], mol_ptr=b["mol_ptr"])
        _, vals, leaves = EG.restate(st, r0["ldj_mol"], kbt, soft, dtype=dtype)
        gr = EG.grads(vals, w, leaves)
        assert np.allclose(gr["ldj"], -w)
        r = FG.flat(FG.reference(layers, dq, b, noise, dt, kind, gr["ldj"], {k: gr[k] for k in FG.KEYS}, dtype=dtype))
        return float((vals.detach().double().numpy() * w).sum()), r, st, r0["ldj_mol"]

    ref_loss, ref, st, ldj_ref = reference(torch.float64)
    loss32, r32, _, _ = reference(torch.float32)
    names = [k for k in ref if not (k.startswith("out.") or k == "ldj_mol")]
    S = float(np.sum(w * EG.scales(st, ldj_ref, kbt, soft)[1]))
    assert abs(loss32 - ref_loss) <= TOL / 2 * S
    assert_all_within({k: normwise(r32[k], ref[k]) for k in names}, GRAD_TOL / 2, "float32 reference gradients")
    errs = {k: normwise(g[k], ref[k]) for k in names}
    print(f"weighted step: w {w}, loss {loss!r} vs {ref_loss!r} (scale {S:.3e}), worst gradient err {max(errs.values()):.2e}")
    assert abs(loss - ref_loss) <= TOL * S
    assert_all_within(errs, GRAD_TOL, "weighted likelihood step gradients")
    _, gm, _ = step(torch.full((M,), 1.0 / M, device=DEV))
    _, gp, _ = step(None, plain=True)
    same = {k: normwise(gm[k], gp[k]) for k in gp}
    print("w = 1 / M vs the plain training step:", max(same.values()))
    assert set(gm) == set(gp)
    assert_all_within(same, 1e-6, "w = 1 / M vs nll(out, ldj)")


def test_in_place_parameter_change_before_backward_raises():
    model, b, noise, _ = _build("base")
    out, ldj_mol = model.forward_grad(_data(b))
    with torch.no_grad():
        model.networks[0].edge_nn[0].weight.mul_(1.0)      # the values stay, the version moves
    with pytest.raises(RuntimeError):
        ldj_mol.sum().backward()
