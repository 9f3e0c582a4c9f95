"""LFIntegrator.reverse_grad on the GPU: values and every gradient of the
differentiable reverse against the float64 restatement of
enflow/flow/dynamics.py:25-37 (tests/_reverse_grad.py).

The loss is a fixed random-weighted sum of the returned g, pos, vel, rev_ldj
(and h where it is differentiable).  Bars, against the float64 restatement:
5e-5 normwise per gradient tensor (the training suite's GRAD_TOL), 1e-5 per
output tensor.  Each case first asserts on the CPU that the float32
restatement is within half of each bar of the float64 one, so the bars measure
the kernels and not the batch's conditioning (seeds chosen for that).
"""
import numpy as np
import pytest
import torch

from _fixtures import normwise, assert_all_within
import _reverse_grad as RG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GRAD_TOL = 5e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _batch(sizes, nf=5, seed=0, chain=False, latent=True):
    """A latent batch (float32-representable): molecules of `sizes` atoms with
    continuous h (one-hot types plus noise), normal g, vel."""
    from enflow_amd.data.synthetic import make_molecules
    b = make_molecules(len(sizes), list(sizes), nf=nf, seed=seed, chain=chain)
    if latent:
        b["h"] = b["h"] + 0.3 * np.random.default_rng(seed + 1000).normal(size=b["h"].shape)
    for k in ("h", "g", "pos", "vel", "box", "r_cut"):
        b[k] = _f32(b[k])
    return b


def _model(nets, dequant=None):
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    return LFIntegrator(nets, dequant, dt=default_dt())


def _egcl(n, nf, hid, seed, **kw):
    from enflow_amd.nn import EGCL
    torch.manual_seed(seed)
    return [EGCL(nf, nf, hid, **kw) for _ in range(n)]


def _prelu():
    m = torch.nn.PReLU(init=0.2)
    m.weight.requires_grad_(False)
    return m


# name -> (model builder, batch builder, names in the loss: h g p(os) v(el) l(dj)); the seeds
# are ones for which the float32 restatement meets half the bars (_reference asserts it)
CASES = {
    "base": (lambda: _model(_egcl(2, 5, 32, 11)), lambda: _batch([5, 9, 22], seed=12), "hgpvl"),
    "h128_argmax": (lambda: _model(_egcl(3, 5, 128, 21), "argmax"), lambda: _batch([9, 22], seed=22), "gpvl"),
    "floor": (lambda: _model(_egcl(2, 5, 32, 31), "floor"), lambda: _batch([7, 22], seed=32), "gpvl"),
    "variants": (lambda: _model(_egcl(2, 5, 64, 41, attention=True, norm_diff=True, tanh=True)),
                 lambda: _batch([9, 22], seed=42), "hgpvl"),
    "gelu": (lambda: _model(_egcl(2, 5, 32, 51, act_fn=torch.nn.GELU())), lambda: _batch([9, 22], seed=52), "hgpvl"),
    "prelu": (lambda: _model(_egcl(2, 5, 32, 61, act_fn=_prelu())), lambda: _batch([9, 22], seed=62), "hgpvl"),
    "n40": (lambda: _model(_egcl(2, 5, 32, 71)), lambda: _batch([40, 22], seed=72), "hgpvl"),
    "n70_chain": (lambda: _model(_egcl(2, 5, 32, 81)), lambda: _batch([70, 22], seed=82, chain=True), "hgpvl"),
    "nf12": (lambda: _model(_egcl(2, 12, 64, 91)), lambda: _batch([9, 22], nf=12, seed=92), "hgpvl"),
}
NAMES = dict(h="h", g="g", p="pos", v="vel", l="ldj")


def _build(name):
    mk_model, mk_batch, use = CASES[name]
    model = mk_model()
    if model.dequantize == "argmax":
        from enflow_amd.nn import ArgMax
        torch.manual_seed(5)
        model.dequantize = ArgMax(model.networks[0].input_nf, model.networks[0].hidden_nf)
    elif model.dequantize == "floor":
        from enflow_amd.nn import Floor
        model.dequantize = Floor()
    return model, mk_batch(), [NAMES[c] for c in use]


def _weights(b, use, seed=3):
    A, M, nf = b["h"].shape[0], len(b["mol_ptr"]) - 1, b["h"].shape[1]
    shapes = dict(h=(A, nf), g=(A, nf), pos=(A, 3), vel=(A, 3), ldj=(M,))
    w = RG.weights({k: shapes[k] for k in use}, seed)
    return {k: _f32(v) for k, v in w.items()}


def _flat(out, gl, gi):
    d = {f"out.{k}": v for k, v in out.items()}
    d.update({f"in.{k}": v for k, v in gi.items()})
    for i, p in enumerate(gl):
        d.update({f"p{i}.{k}": v for k, v in p.items()})
    return d


_REF = {}


def _reference(name, layers, b, dt, w):
    """float64 values and gradients (computed once per case), after the
    float32-restatement check at half the bars."""
    if name not in _REF:
        ref = _flat(*RG.reference(layers, b, dt, w))
        r32 = _flat(*RG.reference(layers, b, dt, w, dtype=torch.float32))
        errs = {k: normwise(r32[k], ref[k]) for k in ref if np.linalg.norm(ref[k]) > 0}
        assert_all_within({k: v for k, v in errs.items() if k.startswith("out.")}, TOL / 2,
                          f"{name}: float32 restatement outputs")
        assert_all_within({k: v for k, v in errs.items() if not k.startswith("out.")}, GRAD_TOL / 2,
                          f"{name}: float32 restatement gradients")
        _REF[name] = ref
    return _REF[name]


def _run_gpu(model, b, w, leaves=True):
    """reverse_grad + backward of the weighted loss on the GPU: (data, rev_ldj,
    output dict, input-gradient dict, per-layer parameter-gradient dicts)."""
    from enflow_amd.data import Data
    model.to(DEV)
    model.zero_grad(set_to_none=True)
    d = Data.from_arrays(b, device=DEV)
    zin = {}
    if leaves:
        for k in RG.KEYS:
            zin[k] = getattr(d, k).requires_grad_(True)
    out, ldj = model.reverse_grad(d)
    outs = dict(h=out.h, g=out.g, pos=out.pos, vel=out.vel, ldj=ldj)
    loss = RG.loss_of(outs, w)
    loss.backward()
    torch.cuda.synchronize()
    gi = {k: (torch.zeros_like(v) if v.grad is None else v.grad).cpu().numpy() for k, v in zin.items()}
    gl = [{k: p.grad.cpu().numpy() for k, p in n.named_parameters() if p.requires_grad and p.grad is not None}
          for n in model.networks]
    return out, ldj, {k: v.detach().cpu().numpy() for k, v in outs.items()}, gi, gl


def _compare(name, ref, use, vals, gi, gl):
    errs = {}
    for k in ("g", "pos", "vel", "ldj") + (("h",) if "h" in use else ()):
        errs[f"out.{k}"] = normwise(vals[k], ref[f"out.{k}"])
    gerr = {}
    got = {f"in.{k}": v for k, v in gi.items()}
    for i, p in enumerate(gl):
        got.update({f"p{i}.{k}": v for k, v in p.items()})
    for k, r in ref.items():
        if k.startswith("out."):
            continue
        assert k in got, f"{name}: no gradient for {k}"
        if np.linalg.norm(r) == 0:
            assert not np.any(got[k]), f"{name}: {k} is exactly zero in the reference"
            continue
        gerr[k] = normwise(got[k], r)
    print(f"{name}: worst output err {max(errs.values()):.2e}, worst gradient err {max(gerr.values()):.2e} "
          f"({max(gerr, key=gerr.get)})")
    assert_all_within(errs, TOL, f"{name}: outputs")
    assert_all_within(gerr, GRAD_TOL, f"{name}: gradients")
    return errs, gerr


def _case(name):
    model, b, use = _build(name)
    layers = RG.model_layers(model)
    w = _weights(b, use)
    ref = _reference(name, layers, b, float(model.dt), w)
    out, ldj, vals, gi, gl = _run_gpu(model, b, w)
    _compare(name, ref, use, vals, gi, gl)
    return model, out, ldj, ref


@pytest.mark.parametrize("name", ["base", "variants", "gelu", "prelu", "n40", "n70_chain", "nf12"])
def test_values_and_gradients_no_dequantiser(name):
    """Every input gradient and every parameter gradient, and the values; the
    returned h is differentiable.  base: molecules of 5, 9 and 22 atoms; n40: the
    33..64-atom backward instance; n70_chain: the large-system backward branch;
    nf12: the 16-feature library."""
    model, out, ldj, _ = _case(name)
    assert out.h.requires_grad and out.g.requires_grad and out.pos.requires_grad and ldj.requires_grad
    if name == "prelu":      # the frozen slope gets no gradient
        assert all(p.grad is None for n in model.networks for p in n.act_fn.parameters())


@pytest.mark.parametrize("name", ["h128_argmax", "floor"])
def test_dequantiser_reverse_passes_no_gradient(name):
    """After ArgMax.reverse / Floor.reverse data.h carries no gradient and the
    dequantiser's parameters get None; the other gradients meet the bar."""
    from oracle import enflow_oracle as O
    model, out, ldj, ref = _case(name)
    assert not out.h.requires_grad and out.h.grad_fn is None
    assert all(p.grad is None for p in model.dequantize.parameters())
    want = O.argmax_reverse(ref["out.h"]) if name == "h128_argmax" else O.floor_reverse(ref["out.h"])
    assert np.array_equal(out.h.cpu().numpy(), want)


@pytest.mark.parametrize("use", [["ldj"], ["pos"]])
def test_one_output_used_upstream(use):
    """Only rev_ldj, or only pos, reaches the loss: the other adjoints arrive as None."""
    model, b, _ = _build("base")
    layers = RG.model_layers(model)
    w = _weights(b, use)
    ref = _reference("base:" + use[0], layers, b, float(model.dt), w)
    _, _, vals, gi, gl = _run_gpu(model, b, w)
    _compare("base:" + use[0], ref, use, vals, gi, gl)


def test_zero_adjoints_give_exactly_zero_gradients():
    model, b, use = _build("base")
    w = {k: np.zeros_like(v) for k, v in _weights(b, use).items()}
    _, _, _, gi, gl = _run_gpu(model, b, w)
    assert all(not np.any(v) for v in gi.values())
    assert all(not np.any(v) for p in gl for v in p.values()) and all(len(p) for p in gl)
    # nothing upstream at all: autograd never enters the backward, every gradient stays None
    from enflow_amd.data import Data
    model.zero_grad(set_to_none=True)
    out, ldj = model.reverse_grad(Data.from_arrays(b, device=DEV))
    (ldj.detach().sum() + next(model.parameters()).sum() * 0).backward()
    assert all(p.grad is None or not torch.any(p.grad) for p in model.parameters())


def _energy(pos, ldj, mol_ptr, soft=0.5):
    """A softened pair potential on the generated positions minus rev_ldj, meaned over molecules."""
    tot = 0.0
    for m in range(len(mol_ptr) - 1):
        x = pos[int(mol_ptr[m]):int(mol_ptr[m + 1])]
        d2 = (x.unsqueeze(1) - x).pow(2).sum(2)
        iu = torch.triu_indices(x.shape[0], x.shape[0], 1)
        r6 = (d2[iu[0], iu[1]] + soft).pow(3)
        tot = tot + 4 * (1 / r6.pow(2) - 1 / r6).sum()
    return (tot - ldj.sum()) / (len(mol_ptr) - 1)


def test_energy_loss_composed_in_torch_and_one_sgd_step():
    """Training by energy: U(x(z)) - rev_ldj written in torch on top of
    reverse_grad; its gradients meet the bar and one small SGD step lowers the
    loss on the same latent batch."""
    from enflow_amd.data import Data
    model, b, _ = _build("base")
    layers = RG.model_layers(model)
    out64, P, leaves = RG.restate(layers, b, float(model.dt))
    ref_loss = _energy(out64["pos"], out64["ldj"], b["mol_ptr"])
    gl, gi = RG.grads_of(ref_loss, P, leaves)
    out32, P32, l32 = RG.restate(layers, b, float(model.dt), dtype=torch.float32)
    gl32, gi32 = RG.grads_of(_energy(out32["pos"], out32["ldj"], b["mol_ptr"]), P32, l32)
    f32 = {f"p{i}.{k}": normwise(gl32[i][k], gl[i][k]) for i in range(len(gl)) for k in gl[i]}
    f32.update({f"in.{k}": normwise(gi32[k], gi[k]) for k in gi})
    assert_all_within(f32, GRAD_TOL / 2, "float32 restatement of the energy gradients")
    model.to(DEV)

    def loss_now(leaf):
        d = Data.from_arrays(b, device=DEV)
        zin = {k: getattr(d, k).requires_grad_(leaf) for k in RG.KEYS}
        o, ldj = model.reverse_grad(d)
        return _energy(o.pos, ldj, b["mol_ptr"]), zin

    loss, zin = loss_now(True)
    loss.backward()
    errs = {f"in.{k}": normwise(zin[k].grad.cpu().numpy(), gi[k]) for k in gi}
    for i, n in enumerate(model.networks):
        errs.update({f"p{i}.{k}": normwise(p.grad.cpu().numpy(), gl[i][k]) for k, p in n.named_parameters()})
    g2 = sum(float((p.grad.double() ** 2).sum()) for p in model.parameters())
    lr = 0.01 * abs(loss.item()) / g2      # a first-order decrease of 1 % of the loss
    with torch.no_grad():
        for p in model.parameters():
            p -= lr * p.grad
    after, _ = loss_now(False)
    print(f"energy loss {loss.item():.6f} (float64 {ref_loss.item():.6f}), worst gradient err "
          f"{max(errs.values()):.2e}; after one SGD step (lr {lr:.3e}) {after.item():.6f}")
    assert abs(loss.item() - ref_loss.item()) <= TOL * abs(ref_loss.item())
    assert_all_within(errs, GRAD_TOL, "energy gradients")
    assert after.item() < loss.item()


def test_backward_is_bitwise_reproducible():
    model, b, use = _build("base")
    w = _weights(b, use)
    _, _, v1, gi1, gl1 = _run_gpu(model, b, w)
    _, _, v2, gi2, gl2 = _run_gpu(model, b, w)
    assert all(np.array_equal(v1[k], v2[k]) for k in v1)
    assert all(np.array_equal(gi1[k], gi2[k]) for k in gi1)
    assert all(np.array_equal(a[k], c[k]) for a, c in zip(gl1, gl2) for k in a)


@pytest.mark.parametrize("name", ["base", "h128_argmax", "n70_chain"])
def test_values_against_the_inference_reverse(name):
    """Under no_grad reverse_grad IS reverse(return_ldj=True) (bitwise); under
    autograd the layer-at-a-time launches agree with the single launch to
    1e-6 normwise (the dequantised h exactly)."""
    from enflow_amd.data import Data
    model, b, _ = _build(name)
    model.to(DEV)
    with torch.no_grad():
        r, rl = model.reverse(Data.from_arrays(b, device=DEV), return_ldj=True)
        n, nl = model.reverse_grad(Data.from_arrays(b, device=DEV))
    for k in RG.KEYS:
        assert torch.equal(getattr(r, k), getattr(n, k)), k
    assert torch.equal(rl, nl)
    g, gl = model.reverse_grad(Data.from_arrays(b, device=DEV))
    assert gl.requires_grad
    errs = {k: normwise(getattr(g, k).detach().cpu().numpy(), getattr(r, k).cpu().numpy()) for k in ("g", "pos", "vel")}
    errs["ldj"] = normwise(gl.detach().cpu().numpy(), rl.cpu().numpy())
    print(f"{name}: layer-at-a-time vs single launch", errs)
    assert_all_within(errs, 1e-6, "values under autograd vs the single launch")
    if model.dequantize is not None:
        assert torch.equal(g.h, r.h)
    # frozen parameters and plain inputs: nothing to differentiate, the single launch again
    for p in model.parameters():
        p.requires_grad_(False)
    f, fl = model.reverse_grad(Data.from_arrays(b, device=DEV))
    assert torch.equal(fl, rl) and torch.equal(f.pos, r.pos) and not fl.requires_grad


def test_small_operands_rerun_with_fp32_gemms():
    """tests/test_gpu_small.py's recipe (features and one layer's edge_nn.0 at
    1e-3: an f16x3 operand entirely below 2^-7): the call is made again with
    fp32 GEMMs (FP32_RERUNS) and the fp32 backward; the bars hold."""
    from enflow_amd import _lib
    scale = 1e-3
    b = _batch([22] * 6, seed=41, latent=False)
    rng = np.random.default_rng(42)
    b["h"] = _f32(np.floor(rng.uniform(0, 3, size=b["h"].shape)) * scale)
    b["g"] = _f32(b["g"] * scale)
    nets = _egcl(3, 5, 64, 43)
    with torch.no_grad():
        nets[1].edge_nn[0].weight.mul_(scale)
        nets[1].edge_nn[0].bias.mul_(scale)
    model = _model(nets)
    use = ["h", "g", "pos", "vel", "ldj"]
    w = _weights(b, use)
    ref = _reference("small", RG.model_layers(model), b, float(model.dt), w)
    n0 = _lib.FP32_RERUNS[0]
    _, _, vals, gi, gl = _run_gpu(model, b, w)
    reruns = _lib.FP32_RERUNS[0] - n0
    print("small operands: fp32 re-runs", reruns)
    assert reruns >= 1
    _compare("small", ref, use, vals, gi, gl)


def test_in_place_parameter_change_before_backward_raises():
    from enflow_amd.data import Data
    model, b, _ = _build("base")
    model.to(DEV)
    out, ldj = model.reverse_grad(Data.from_arrays(b, device=DEV))
    with torch.no_grad():
        model.networks[0].edge_nn[0].weight.mul_(1.5)
    with pytest.raises(RuntimeError):
        ldj.sum().backward()


def test_untrainable_configurations_are_refused():
    from enflow_amd.data import Data
    model = _model(_egcl(2, 5, 32, 3, act_fn=torch.nn.PReLU())).to(DEV)     # a trainable slope
    b = _batch([9, 22], seed=4)
    with pytest.raises(NotImplementedError):
        model.reverse_grad(Data.from_arrays(b, device=DEV))
    model = _model(_egcl(1, 17, 32, 3)).to(DEV)
    with pytest.raises(NotImplementedError):
        model.reverse_grad(Data.from_arrays(_batch([9], nf=17, seed=4), device=DEV))


def test_forward_of_reverse_grad_is_the_identity_with_identity_vjp():
    """No dequantiser: forward(reverse_grad(z)) = z and its vjp with a weight w
    is w (1e-4 normwise: the chain runs through two fp32 backwards, twice the
    gradient bar; positions compared modulo the box, which both directions wrap
    into).  Measured on the MI355X: values <= 5e-8, vjp <= 9e-8."""
    from enflow_amd.data import Data
    model, b, use = _build("base")
    model.to(DEV)
    w = _weights(b, ["h", "g", "pos", "vel"], seed=9)
    d = Data.from_arrays(b, device=DEV)
    zin = {k: getattr(d, k).requires_grad_(True) for k in RG.KEYS}
    z0 = {k: v.detach().clone() for k, v in zin.items()}
    x, _ = model.reverse_grad(d)
    back, _ = model(x)
    loss = RG.loss_of({k: getattr(back, k) for k in RG.KEYS}, w)
    model.zero_grad(set_to_none=True)
    loss.backward()
    val = {k: normwise(getattr(back, k).detach().cpu().numpy(), z0[k].cpu().numpy()) for k in ("h", "g", "vel")}
    # the flow wraps positions into the periodic box (data.pbc()): z's positions modulo the box
    dpos = back.pos.detach().cpu().double().numpy() - z0["pos"].cpu().double().numpy()
    dpos -= np.round(dpos / b["box"]) * b["box"]
    val["pos"] = float(np.linalg.norm(dpos) / np.linalg.norm(z0["pos"].cpu().double().numpy()))
    vjp = {k: normwise(zin[k].grad.cpu().numpy(), w[k]) for k in RG.KEYS}
    pg = max(float(p.grad.abs().max()) for p in model.parameters())
    print("forward(reverse_grad(z)) vs z:", val, "; vjp vs w:", vjp, "; largest |parameter gradient| (0 ideally):", pg)
    assert_all_within(val, 1e-4, "forward(reverse_grad(z)) vs z")
    assert_all_within(vjp, 1e-4, "vjp of the identity")
