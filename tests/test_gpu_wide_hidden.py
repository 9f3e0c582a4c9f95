"""hidden_nf 129..256 on the GPU (csrc/enflow_wide.hip): LFIntegrator forward /
reverse, EGCL and ArgMax alone, against the float64 oracle on the same
float32-rounded inputs.  Bars: every output tensor and log|detJ| <= 1e-5
normwise; each case first asserts that the oracle evaluated in float32 on the
CPU is within half the bar (the bar is then reachable in fp32 at all);
dequantised h of a reverse is exact.

Cases run at gemm_precision "f16x3" (the default) and "f32", and with the row
blocks forced to 8 / 16 / 32 rows (ENFLOW_LARGE_ROWS; the host picks 4 for
batches this small), so that a block's pair words exceed one pass of 512.
"""
import numpy as np
import pytest
import torch

from _fixtures import normwise, scalar_rel, assert_all_within, dequant_params, state  # noqa: F401
from _wide import cast, f32, golden_model, oracle_params
from oracle import enflow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
KEYS = ("h", "g", "pos", "vel")


def _data(b):
    from enflow_amd.data import Data
    return Data.from_arrays(b, device=DEV)


def _errs(got, ref, keys=KEYS):
    return {k: normwise(getattr(got, k).cpu().numpy(), ref[k]) for k in keys}


def _refs(model, b, noise, kind):
    """float64 oracle forward (state, ldj) after asserting its float32 evaluation at half the bar."""
    res = {}
    for dt in (np.float64, np.float32):
        layers = [oracle_params(n, dt) for n in model.networks]
        if kind == "argmax":
            dq = oracle_params(model.dequantize, dt)
        elif kind == "floor":
            dq = 1.0
        else:
            dq = 0.0
        nz = np.zeros_like(b["h"]) if noise is None else noise
        res[dt] = O.lf_forward(layers, dq, cast(b, dt), nz.astype(dt), dt(model.dt),
                               dequant_kind="argmax" if kind == "argmax" else "floor")
    (r64, l64), (r32, l32) = res[np.float64], res[np.float32]
    e = {k: normwise(r32[k], r64[k]) for k in KEYS}
    e["ldj"] = scalar_rel(l32, l64) if l64 != 0 else abs(l32)
    assert_all_within(e, TOL / 2, "float32 CPU evaluation of the forward")
    return r64, l64


def _rev_ref(model, st, kind):
    res = {}
    for dt in (np.float64, np.float32):
        layers = [oracle_params(n, dt) for n in model.networks]
        res[dt] = O.lf_reverse(layers, cast(st, dt), dt(model.dt), dequant_kind=kind)
    e = {k: normwise(res[np.float32][k], res[np.float64][k]) for k in ("g", "pos", "vel")}
    assert_all_within(e, TOL / 2, "float32 CPU evaluation of the reverse")
    return res[np.float64]


def _check_flow(model, b, kind, seed, prec="f16x3", reruns=0):
    """forward and reverse of the forward's output vs the oracle; returns (out, ldj, ref, ref_ldj).
    reruns: fp32 re-runs the forward must take (_lib.FP32_RERUNS)."""
    from enflow_amd import _lib
    model.gemm_precision = prec
    d = _data(b)
    noise = None
    if kind == "argmax":
        noise = torch.randn(d.h.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    elif kind == "floor":
        noise = torch.rand(d.h.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    nz = None if noise is None else noise.cpu().double().numpy()
    ref, ref_ldj = _refs(model, b, nz, kind)
    r0 = _lib.FP32_RERUNS[0]
    with torch.no_grad():
        out, ldj = model(d, noise=noise)
    assert _lib.FP32_RERUNS[0] - r0 == reruns, "fp32 re-runs of the forward"
    e = _errs(out, ref)
    e["ldj"] = scalar_rel(float(ldj), ref_ldj) if ref_ldj != 0 else abs(float(ldj))
    print(f"{kind} {prec} forward:", {k: f"{v:.2e}" for k, v in e.items()})
    assert_all_within(e, TOL, "forward")
    # reverse of the GPU's own (float32) forward output, continuous part vs the oracle
    st = {k: getattr(out, k).cpu().double().numpy() for k in KEYS}
    st.update(box=b["box"], r_cut=b["r_cut"], mol_ptr=b["mol_ptr"])
    rref = _rev_ref(model, st, "none")
    with torch.no_grad():
        back = model.reverse(out.clone())
    e = _errs(back, rref, ("g", "pos", "vel"))
    print(f"{kind} reverse:", {k: f"{v:.2e}" for k, v in e.items()})
    assert_all_within(e, TOL, "reverse")
    hb = back.h.cpu().numpy()
    if kind == "argmax":
        want = O.argmax_reverse(rref["h"])
        assert hb.shape == want.shape and np.array_equal(hb, want)
    elif kind == "none":
        assert normwise(hb, rref["h"]) <= TOL
    return out, ldj, ref, ref_ldj, back


def _rev_ldj_ref(model, b, out):
    """The reverse's per-molecule log|detJ| of the GPU state `out`: -sum of Q per molecule, Q where
    the reverse evaluates it; {float64: [M], float32: [M]} after asserting the float32 evaluation
    at half the bar (normwise over the vector)."""
    st = {k: getattr(out, k).cpu().double().numpy() for k in KEYS}
    st.update(box=b["box"], r_cut=b["r_cut"], mol_ptr=b["mol_ptr"])
    want = {}
    for dt in (np.float64, np.float32):
        s = cast(st, dt)
        tot = np.zeros(len(b["mol_ptr"]) - 1)
        for p in reversed([oracle_params(n, dt) for n in model.networks]):
            s["h"] = s["h"] - s["g"] * dt(model.dt)
            s["pos"] = O.apply_pbc(s["pos"] - s["vel"] * dt(model.dt), s["box"])
            q, f, g = O._layer(p, s["h"], s["pos"], s["box"], s["r_cut"], s["mol_ptr"], 1.0)
            s["g"] = s["g"] - g * dt(model.dt)
            s["vel"] = (s["vel"] - f * dt(model.dt)) / np.exp(q)
            tot -= np.add.reduceat(q[:, 0].astype(np.float64), s["mol_ptr"][:-1])
        want[dt] = tot
    assert normwise(want[np.float32], want[np.float64]) <= TOL / 2
    return want


def _model(hid, nf, kind, seed, n_layers=2, **kw):
    from enflow_amd.nn import EGCL, ArgMax, Floor
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    torch.manual_seed(seed)
    nets = [EGCL(nf, nf, hid, **kw) for _ in range(n_layers)]
    dq = ArgMax(nf, hid) if kind == "argmax" else (Floor() if kind == "floor" else None)
    return LFIntegrator(nets, dq, dt=default_dt()).to(DEV)


@pytest.fixture(params=[None, 8, 16, 32], ids=lambda r: f"rows{r or 'auto'}")
def rows(request, monkeypatch):
    """Rows per block of the large-system kernels (None: the host's choice, 4 at these sizes)."""
    if request.param is not None:
        monkeypatch.setenv("ENFLOW_LARGE_ROWS", str(request.param))
    return request.param


# 1. the reference-made golden at width 256
@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_golden_batch(prec, rows):
    from enflow_amd.flow import Alchemical_NLL
    from _fixtures import data_from_fixture
    model, inp, gold = golden_model(DEV)
    model.gemm_precision = prec
    eps = torch.tensor(inp["eps"], device=DEV)
    with torch.no_grad():
        out, ldj = model(data_from_fixture(inp, DEV), noise=eps)
        nll = Alchemical_NLL(kBT=float(inp["kBT"]), softening=float(inp["softening"]))(out, ldj)
    e = _errs(out, gold)
    e["ldj"] = scalar_rel(float(ldj), float(gold["ldj"]))
    e["nll"] = scalar_rel(float(nll), float(gold["nll"]))
    print("golden forward:", {k: f"{v:.2e}" for k, v in e.items()})
    assert_all_within(e, TOL, "golden forward")
    # reverse of the reference's own forward output (float32-rounded), vs the oracle on the same values
    st = {k: gold[k].astype(np.float32).astype(np.float64) for k in KEYS}
    st.update(box=inp["box"].astype(np.float64), r_cut=inp["r_cut"].astype(np.float64), mol_ptr=inp["mol_ptr"])
    rref = _rev_ref(model, st, "none")
    from enflow_amd.data import Data
    with torch.no_grad():
        back = model.reverse(Data.from_arrays(st, device=DEV))
    e = _errs(back, rref, ("g", "pos", "vel"))
    e.update({"gold_" + k: normwise(getattr(back, k).cpu().numpy(), gold["rev_" + k]) for k in ("g", "pos", "vel")})
    assert_all_within(e, TOL, "golden reverse")
    assert np.array_equal(back.h.cpu().numpy(), gold["rev_h"])
    # round trip reverse(forward(x)) = x, at the large-system round-trip test's bar (1e-4)
    with torch.no_grad():
        rt = model.reverse(out.clone())
    hb = rt.h.cpu().numpy()      # the reference's one-hot is max index + 1 wide (helpers.py:43-52)
    assert np.array_equal(hb, inp["h"][:, :hb.shape[1]]) and not inp["h"][:, hb.shape[1]:].any()
    # vel as that test compares it, pos up to the periodic wrap the flow applies.  g is printed,
    # not asserted: the input positions are not wrapped into the box, so the reverse's first layer
    # sees other periodic images than the forward's did and the reference's own float64 round
    # trip of g is off by 8.9e-4 of its scale on this batch
    box = inp["box"].astype(np.float64)
    dpos = O.apply_pbc(rt.pos.cpu().double().numpy() - inp["pos"], box)
    gs = max(float(np.max(np.abs(out.g.cpu().numpy()))), 1e-30)
    rte = {"vel": normwise(rt.vel.cpu().numpy(), inp["vel"]),
           "pos": float(np.max(np.abs(dpos)) / np.max(np.abs(inp["pos"]))),
           "g": float(np.max(np.abs(rt.g.cpu().numpy() - inp["g"])) / gs)}
    print("round trip:", rte)
    rte.pop("g")
    assert_all_within(rte, 1e-4, "round trip")


# 2. padded width, Floor, several row blocks, a ragged tail.  At a 5 A cutoff the 70-atom chain has
# ~1300 pair words per 32 rows (multiplicities up to 6): three passes of 512 at 32 rows per block,
# two at 16, one at 8 and 4; tiles then span many rows and every row index 0..31 is used
@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_h160_floor_chains(prec, rows):
    from enflow_amd.data.synthetic import make_molecules
    b = f32(make_molecules(2, [40, 70], nf=5, seed=160, chain=True, r_cut_ang=5.0))
    b2 = f32(make_molecules(1, [22], nf=5, seed=161))
    for k in KEYS + ("box",):
        b[k] = np.concatenate([b[k], b2[k]])
    b["r_cut"] = np.concatenate([b["r_cut"], b2["r_cut"]])
    b["mol_ptr"] = np.concatenate([b["mol_ptr"], b["mol_ptr"][-1:] + b2["mol_ptr"][1:]])
    b["h"] = np.floor(np.random.default_rng(3).uniform(0, 3, size=b["h"].shape))
    if rows == 32:      # the construction's premise: a block past two passes
        from enflow_amd import _lib
        d = _data(b)
        ws = _lib.large_workspace(3, 132, 70, 1, DEV)
        npairs = torch.zeros(132, dtype=torch.int32, device=DEV)
        words = torch.zeros(132 * 70, dtype=torch.int32, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.check(_lib.lib().enflow_neighbour_pairs_large_f32(
            3, 132, 70, _lib.ptr(d.edges.mol_ptr), _lib.ptr(torch.as_tensor(b["r_cut"], dtype=torch.float32, device=DEV)),
            _lib.ptr(d.edges.box.float().contiguous()), _lib.ptr(d.edges.pos.float().contiguous()), _lib.ptr(npairs),
            _lib.ptr(words), _lib.ptr(err), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)), "pairs")
        assert int(npairs[40:72].sum()) > 2 * 512
    _check_flow(_model(160, 5, "floor", 160), b, "floor", 2, prec)


# 3. the 16-feature library, no dequantiser
def test_h256_nf12_no_dequantiser():
    from enflow_amd.data.synthetic import make_molecules
    b = f32(make_molecules(3, [9, 22, 13], nf=12, seed=12))
    b["h"] = np.random.default_rng(4).normal(size=b["h"].shape).astype(np.float32).astype(np.float64)
    _check_flow(_model(256, 12, "none", 12), b, "none", 0)
    _check_flow(_model(256, 12, "none", 12), b, "none", 0, "f32")


# 4. every constructor variant with GELU, a Tanh ArgMax
def test_h256_variants_gelu_tanh_argmax():
    from torch import nn
    from enflow_amd.data.synthetic import make_molecules
    b = f32(make_molecules(3, [22, 5, 17], nf=5, seed=44))
    _check_flow(_variant_model(), b, "argmax", 5)


def _variant_model():
    from torch import nn
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    torch.manual_seed(44)
    nets = [EGCL(5, 5, 256, attention=True, norm_diff=True, tanh=True, act_fn=nn.GELU()) for _ in range(2)]
    return LFIntegrator(nets, ArgMax(5, 256, act_fn=nn.Tanh()), dt=default_dt()).to(DEV)


# 5. per-molecule log|detJ| in both directions
def test_per_molecule_ldj():
    from enflow_amd.data.synthetic import make_molecules
    b = f32(make_molecules(3, [22, 40, 9], nf=5, seed=55))
    model = _model(256, 5, "argmax", 55)
    d = _data(b)
    noise = torch.randn(d.h.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    with torch.no_grad():
        out, ldj = model(_data(b), noise=noise)
        out2, ldj_mol = model(_data(b), noise=noise, per_molecule=True)
    assert ldj_mol.shape == (3,)
    assert abs(float(ldj_mol.double().sum()) - float(ldj)) <= 1e-6 * max(abs(float(ldj)), 1.0)
    for k in KEYS:
        assert torch.equal(getattr(out, k), getattr(out2, k))
    want = _rev_ldj_ref(model, b, out)[np.float64]
    with torch.no_grad():
        _, rev = model.reverse(out.clone(), return_ldj=True)
    assert normwise(rev.cpu().numpy(), want) <= TOL


# 6. bitwise reproducible
def test_bitwise_reproducible():
    from enflow_amd.data.synthetic import make_molecules
    b = f32(make_molecules(3, [22, 40, 9], nf=5, seed=66))
    model = _model(256, 5, "argmax", 66)
    noise = torch.randn((71, 5), device=DEV, generator=torch.Generator(DEV).manual_seed(7))
    with torch.no_grad():
        o1, l1 = model(_data(b), noise=noise)
        o2, l2 = model(_data(b), noise=noise)
        r1 = model.reverse(o1.clone())
        r2 = model.reverse(o2.clone())
    assert torch.equal(l1, l2)
    for k in KEYS:
        assert torch.equal(getattr(o1, k), getattr(o2, k)), k
        assert torch.equal(getattr(r1, k), getattr(r2, k)), k


# 8. the modules alone
def test_egcl_and_argmax_alone():
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.data.synthetic import make_molecules
    b = f32(make_molecules(3, [22, 40, 9], nf=5, seed=88))
    b["h"] = np.random.default_rng(8).normal(size=b["h"].shape).astype(np.float32).astype(np.float64)
    torch.manual_seed(88)
    net, am = EGCL(5, 5, 256).to(DEV), ArgMax(5, 256).to(DEV)
    d = _data(b)
    with torch.no_grad():
        q, f, g = net(d.h, d.edges)
    ref = {}
    for dt in (np.float64, np.float32):
        c = cast(b, dt)
        ref[dt] = O._layer(oracle_params(net, dt), c["h"], c["pos"], c["box"], c["r_cut"], c["mol_ptr"], 1.0)
    e32 = [normwise(a, r) for a, r in zip(ref[np.float32], ref[np.float64])]
    assert_all_within(e32, TOL / 2, "float32 CPU evaluation of EGCL")
    e = [normwise(a.cpu().numpy(), r) for a, r in zip((q, f, g), ref[np.float64])]
    print("EGCL alone:", e)
    assert_all_within(e, TOL, "EGCL(5, 5, 256)")
    hq = np.eye(5)[np.random.default_rng(9).integers(0, 5, size=71)]
    eps = torch.randn((71, 5), device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    with torch.no_grad():
        z, lq = am(torch.tensor(hq, dtype=torch.float32, device=DEV), noise=eps)
    z64, lq64 = O.argmax_forward(oracle_params(am), hq, eps.cpu().double().numpy())
    z32, lq32 = O.argmax_forward(oracle_params(am, np.float32), hq.astype(np.float32), eps.cpu().numpy())
    assert normwise(z32, z64) <= TOL / 2 and scalar_rel(lq32, lq64) <= TOL / 2
    assert normwise(z.cpu().numpy(), z64) <= TOL and scalar_rel(float(lq), lq64) <= TOL


# 9. refusals on the device
def test_refusals():
    from enflow_amd.nn import EGCL
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import make_molecules, default_dt
    b = f32(make_molecules(1, [9], nf=5, seed=9))
    with pytest.raises(NotImplementedError, match="hidden_nf <= 256"):
        LFIntegrator([EGCL(5, 5, 257)], None, dt=default_dt()).to(DEV)(_data(b))
    model = LFIntegrator([EGCL(5, 5, 256)], None, dt=default_dt()).to(DEV)
    with pytest.raises(NotImplementedError, match="inference only at hidden_nf > 128: call under torch.no_grad()"):
        model(_data(b))


# 7. the f16x3 guards at both ends of the range
def test_small_operands_rerun_in_fp32():
    """Inputs scaled to 1e-3: edge_nn.0's input and vel_scaling_nn.0's never reach 2^-7, the
    f16x3 launch flags ENFLOW_ERR_SMALL and the host re-runs the batch once with fp32 GEMMs."""
    from enflow_amd.data.synthetic import make_molecules
    b = make_molecules(3, [22, 9, 13], nf=5, seed=77)
    b["h"] = np.floor(np.random.default_rng(7).uniform(0, 3, size=b["h"].shape))
    for k in ("h", "g", "pos", "vel", "box", "r_cut"):
        b[k] = b[k] * 1e-3
    b = f32(b)
    model = _model(256, 5, "none", 77)
    _check_flow(model, b, "none", 0, "f16x3", reruns=1)
    _check_flow(model, b, "none", 0, "f32", reruns=0)


@pytest.mark.parametrize("scale", [3e4, 1e6])
def test_f16x3_range_guard_h256(scale):
    """tests/test_gpu_parity.py::test_f16x3_range_guard's construction at hidden_nf 256: features
    up to `scale`, coord_nn.2 x300, a tanh layer, vel_scaling_nn.2 zeroed so the float64 reference
    stays finite.  The module call meets the bar at f32 and at f16x3 (re-run in fp32 on the flag);
    the raw f16x3 launch flags ENFLOW_ERR_RANGE or returns the oracle's result, never a finite
    wrong one, and flags at 1e6 (past the fp16 range)."""
    from enflow_amd import _lib
    from enflow_amd.nn import EGCL, Floor
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import make_molecules, default_dt
    b = f32(make_molecules(4, 22, nf=4, seed=13))
    b["h"] = np.floor(np.random.default_rng(14).uniform(0, scale, size=b["h"].shape)).astype(np.float32).astype(np.float64)
    torch.manual_seed(15)
    nets = [EGCL(4, 4, 256), EGCL(4, 4, 256, tanh=True)]
    with torch.no_grad():
        for n in nets:
            n.vel_scaling_nn[2].weight.zero_()
            n.vel_scaling_nn[2].bias.fill_(0.01)
            n.coord_nn[2].weight.mul_(300.0)
    model = LFIntegrator(nets, Floor(), dt=default_dt()).to(DEV)
    u = torch.rand(b["h"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(16))
    layers = [oracle_params(n) for n in model.networks]
    ref, ref_ldj = O.lf_forward(layers, 1.0, b, u.cpu().double().numpy(), model.dt, dequant_kind="floor")
    assert all(np.isfinite(ref[k]).all() for k in KEYS)
    for prec in ("f32", "f16x3"):
        model.gemm_precision = prec
        with torch.no_grad():
            o, ldj = model(_data(b), noise=u)
        e = _errs(o, ref)
        e["ldj"] = scalar_rel(float(ldj), ref_ldj)
        print(f"range guard {scale:g} {prec}:", {k: f"{v:.2e}" for k, v in e.items()})
        assert_all_within(e, TOL, f"{prec} module call")
    s = model._state(_data(b))
    ldj_mol, ldj = torch.empty(4, device=DEV), torch.empty(1, device=DEV)
    st = torch.zeros(2, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        model.forward_buffers(s["h"], s["g"], s["pos"], s["vel"], s["box"], s["r_cut"], s["mol_ptr"], s["max_n"],
                              u, ldj_mol, ldj, st[:1], src=s["src"], ticket=st[1:])
    flagged = bool(int(st[0].item()) & _lib.ERR_RANGE)
    if not flagged:
        raw = {k: normwise(s[k].cpu().numpy(), ref[k], allow_nonfinite=True) for k in KEYS}
        assert_all_within(raw, TOL, "unflagged raw f16x3 launch")
    assert flagged or scale < 6.5e4, "fp16 overflow not flagged"


def test_bf16_runs_f16x3_with_a_warning():
    from enflow_amd.data.synthetic import make_molecules
    b = f32(make_molecules(2, [9, 13], nf=5, seed=99))
    model = _model(256, 5, "none", 99)
    with torch.no_grad():
        o1, l1 = model(_data(b))
        model.gemm_precision = "bf16"
        with pytest.warns(RuntimeWarning, match="bf16.*runs f16x3"):
            o2, l2 = model(_data(b))
    assert torch.equal(l1, l2) and all(torch.equal(getattr(o1, k), getattr(o2, k)) for k in KEYS)
