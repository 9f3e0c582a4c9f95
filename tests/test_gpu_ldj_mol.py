"""Per-molecule log-densities on the GPU: LFIntegrator.reverse(return_ldj=True),
LFIntegrator.forward(per_molecule=True), Alchemical_NLL.per_molecule / .potential.

Reference: the float64 oracle (oracle/enflow_oracle.py, pinned to the
reference's goldens).  Forward values and losses come from the oracle's own
lf_forward / alchemical_nll / lj_potential on ONE-molecule states; the reverse
value is restated here from the public pieces lf_reverse itself uses
(apply_pbc, batch_edges, coord_diff, egcl_forward), summing -Q per molecule,
and the restatement's final state must equal lf_reverse's exactly.

Bars (the project's 1e-5): normwise over the [M] vector, and per element
|got - ref| <= 1e-5 * S_m with S_m the sum of the absolute values of the terms
the element sums (a plain relative error would divide by a sum that may
cancel).  bf16: BF16_TOL of tests/test_gpu_parity.py.  For every batch the
same restatement in float32 on the CPU is first asserted to stay within HALF
the bar of the float64 one (the "floor" convention of
tests/test_gpu_grad_edges.py), so the bar tests the kernels, not the inputs.

Two-layer models, hidden 32 unless stated."""
import math

import numpy as np
import pytest
import torch

from oracle import enflow_oracle as O
from _fixtures import normwise
from test_gpu_parity import BF16_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
L2PI = math.log(2.0 * math.pi)
FLOATS = ("h", "g", "pos", "vel", "box", "r_cut")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------
# batches, models, oracle restatements
# ---------------------------------------------------------------------------
def _f32(b):
    out = dict(b)
    for k in FLOATS:
        out[k] = np.asarray(b[k], dtype=np.float32).astype(np.float64)
    return out


_BATCHES = {}


def _batch(sizes, seed, nf=5):
    """Ragged batch, float32-representable float64 arrays (cached, never modified).
    Molecules past the fused kernels' 256 atoms are LJ boxes (the large-system path)."""
    key = (tuple(sizes), seed, nf)
    if key not in _BATCHES:
        from enflow_amd.data.synthetic import make_molecules, make_lj_systems
        if max(sizes) > 256:
            b = make_lj_systems(list(sizes), nf=nf, seed=seed)
        else:
            b = make_molecules(len(sizes), list(sizes), nf=nf, seed=seed)
        _BATCHES[key] = _f32(b)
    return _BATCHES[key]


def _model(kind, hid=32, nf=5, seed=11, prec="f16x3", scale=1.0, **egcl_kw):
    from enflow_amd.nn import EGCL, ArgMax, Floor
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    torch.manual_seed(seed)
    nets = [EGCL(nf, nf, hid, **egcl_kw) for _ in range(2)]
    dq = ArgMax(nf, hid) if kind == "argmax" else Floor(dequant_scale=scale) if kind == "floor" else None
    model = LFIntegrator(nets, dq, dt=default_dt()).to(DEV)
    model.gemm_precision = prec
    return model


def _layers(model, dtype=np.float64):
    out = []
    for n in model.networks:
        p = {k: v.detach().cpu().double().numpy().astype(dtype) for k, v in n.state_dict().items()}
        p["flags"] = (bool(n.attention), bool(n.norm_diff), bool(n.tanh))
        out.append(p)
    return out


def _dq(model, dtype=np.float64):
    return {k: v.detach().cpu().double().numpy().astype(dtype) for k, v in model.dequantize.state_dict().items()}


def _cast(st, dtype):
    s = {k: np.asarray(st[k], dtype=dtype) for k in FLOATS}
    s["mol_ptr"] = np.asarray(st["mol_ptr"], dtype=np.int64)
    return s


def _one(st, m, extra=None):
    """Molecule m of a batch state as a batch of one."""
    a0, a1 = int(st["mol_ptr"][m]), int(st["mol_ptr"][m + 1])
    s = {k: st[k][a0:a1] for k in ("h", "g", "pos", "vel", "box")}
    s["r_cut"] = st["r_cut"][m:m + 1]
    s["mol_ptr"] = np.array([0, a1 - a0], dtype=np.int64)
    return (s, extra[a0:a1]) if extra is not None else s


def _layer(p, s):
    row, col, eb = O.batch_edges(s["pos"], s["box"], s["r_cut"], s["mol_ptr"])
    return O.egcl_forward(p, s["h"], row, col, O.coord_diff(s["pos"], row, col, eb))


def rev_restated(layers, state, dt, dtype=np.float64):
    """lf_reverse's loop (dynamics.py:26-35) from its public pieces, with the
    per-molecule sum of -Q: (final continuous state, rev_ldj [M], S [M] = sum |Q|)."""
    s = _cast(state, dtype)
    ptr = s["mol_ptr"]
    M = len(ptr) - 1
    ldj, S = np.zeros(M), np.zeros(M)
    for p in reversed(layers):
        s["h"] = s["h"] - s["g"] * dt
        s["pos"] = O.apply_pbc(s["pos"] - s["vel"] * dt, s["box"])
        q, f, g = _layer(p, s)
        s["g"] = s["g"] - g * dt
        s["vel"] = (s["vel"] - f * dt) / np.exp(q)
        for m in range(M):
            qm = q[int(ptr[m]):int(ptr[m + 1])].astype(np.float64)
            ldj[m] -= float(np.sum(qm))
            S[m] += float(np.sum(np.abs(qm)))
    return s, ldj, S


def fwd_one_restated(layers, dq, st1, noise1, dt, kind, dtype=np.float64, scale=1.0):
    """lf_forward (dynamics.py:10-24) of a one-molecule state from its public
    pieces: (ldj, S) with S = |log q| + sum |Q|."""
    s = _cast(st1, dtype)
    lq = 0.0
    if kind == "argmax":
        s["h"], lq = O.argmax_forward(dq, s["h"], np.asarray(noise1, dtype=dtype))
    elif kind == "floor":
        s["h"], lq = O.floor_forward(s["h"], np.asarray(noise1, dtype=dtype), dtype(scale))
    ldj, S = float(lq), abs(float(lq))
    for p in layers:
        q, f, g = _layer(p, s)
        s["vel"] = np.exp(q) * s["vel"] + f * dt
        s["g"] = s["g"] + g * dt
        s["pos"] = O.apply_pbc(s["pos"] + s["vel"] * dt, s["box"])
        s["h"] = s["h"] + s["g"] * dt
        ldj = ldj + float(np.sum(q))
        S += float(np.sum(np.abs(q.astype(np.float64))))
    return ldj, S


def _floor_ok(what, v32, v64, S, bar=TOL):
    """The float32 restatement within half the bar of the float64 one."""
    v32, v64, S = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (v32, v64, S))
    nw = normwise(v32, v64)
    worst = float(np.max(np.abs(v32 - v64) / np.maximum(S, 1e-300)))
    print(f"{what}: float32 restatement vs float64: normwise {nw:.2e}, worst element / S {worst:.2e}")
    assert nw <= bar / 2 and worst <= bar / 2, f"{what}: the float32 floor exceeds half the bar; choose another seed"


def _within(what, got, ref, S, bar=TOL):
    got, ref, S = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (got, ref, S))
    nw = normwise(got, ref)
    el = np.abs(got - ref) / np.maximum(S, 1e-300)
    print(f"{what}: normwise {nw:.2e}, worst element / S {float(np.max(el)):.2e} (bar {bar:g})")
    assert np.all(np.isfinite(got)), f"{what}: non-finite values"
    assert nw <= bar, f"{what}: normwise {nw:.2e} over {bar:g}"
    assert np.all(el <= bar), f"{what}: elements over {bar:g} * S_m: {el}"


_REV_REF = {}


def _rev_ref(model, st, key):
    """(rev_ldj, S) of the float64 restatement for a model / state, checked
    against lf_reverse (same computation) and the float32 floor; cached."""
    if key not in _REV_REF:
        fin, ldj, S = rev_restated(_layers(model), st, model.dt)
        ref = O.lf_reverse(_layers(model), st, model.dt, dequant_kind="none")
        for k in ("h", "g", "pos", "vel"):
            assert np.array_equal(fin[k], ref[k]), f"the restatement's final {k} differs from lf_reverse's"
        _, l32, _ = rev_restated(_layers(model, np.float32), st, np.float32(model.dt), np.float32)
        _floor_ok(f"reverse {key}", l32, ldj, S)
        _REV_REF[key] = (ldj, S)
    return _REV_REF[key]


def _data(st):
    from enflow_amd.data import Data
    return Data.from_arrays(st, device=DEV)


def _state_of(d, b):
    st = {k: getattr(d, k).detach().cpu().double().numpy() for k in ("h", "g", "pos", "vel")}
    st.update(box=b["box"], r_cut=b["r_cut"], mol_ptr=b["mol_ptr"])
    return st


SEEDS = {(1, 2, 22, 32): 21, (33, 64): 22, (65, 100): 23, (257, 3): 24, (22, 32): 25, (2, 22): 26}


# ---------------------------------------------------------------------------
# 1. reverse(return_ldj=True) against the restated oracle
# ---------------------------------------------------------------------------
REV_CASES = [((1, 2, 22, 32), k, p, None) for k in ("argmax", "floor", "none") for p in ("f16x3", "f32")]
REV_CASES += [(s, "argmax", p, None) for s in ((33, 64), (65, 100), (257, 3)) for p in ("f16x3", "f32")]
# small batches run the 8-wave latency instance by default: the 4-wave one as well
REV_CASES += [((1, 2, 22, 32), "argmax", "f16x3", "4-wave")]


@pytest.mark.parametrize("sizes,kind,prec,instance", REV_CASES)
def test_reverse_ldj_vs_oracle(sizes, kind, prec, instance):
    from enflow_amd import _lib
    b = _batch(sizes, SEEDS[sizes])
    model = _model(kind, prec=prec)
    ref, S = _rev_ref(model, b, (sizes, 5, 32))
    prev = _lib.set_latency_threshold(0) if instance == "4-wave" else None
    try:
        with torch.no_grad():
            out, rev = model.reverse(_data(b), return_ldj=True)
    finally:
        if instance == "4-wave":
            _lib.set_latency_threshold(-1 if prev is None else prev)
    assert rev.shape == (len(sizes),) and rev.dtype == torch.float32
    _within(f"rev_ldj {sizes} {kind} {prec} {instance or ''}", rev.cpu().numpy(), ref, S)
    assert abs(ref[list(sizes).index(min(sizes))]) > 0      # (a one-atom molecule has no pairs, its Q is not zero)


def test_reverse_ldj_bf16():
    sizes = (22, 32)
    b = _batch(sizes, SEEDS[sizes])
    model = _model("argmax", prec="bf16")
    ref, S = _rev_ref(model, b, (sizes, 5, 32))
    with torch.no_grad():
        _, rev = model.reverse(_data(b), return_ldj=True)
    _within(f"rev_ldj {sizes} bf16", rev.cpu().numpy(), ref, S, bar=BF16_TOL)


def test_reverse_ldj_variant_layers():
    """Layers with constructor variants (attention, tanh): the variant-capable RLDJ instances."""
    sizes = (22, 32)
    b = _batch(sizes, SEEDS[sizes])
    model = _model("argmax", attention=True, tanh=True)
    ref, S = _rev_ref(model, b, (sizes, 5, 32, "att+tanh"))
    with torch.no_grad():
        plain = model.reverse(_data(b))
        out, rev = model.reverse(_data(b), return_ldj=True)
    for k in ("h", "g", "pos", "vel"):
        assert torch.equal(getattr(out, k), getattr(plain, k)), k
    _within(f"rev_ldj {sizes} attention + tanh", rev.cpu().numpy(), ref, S)


def test_reverse_ldj_node_nf_16():
    """node_nf 16: the second library (libenflow_hip_nf16.so)."""
    sizes = (2, 22)
    b = _batch(sizes, SEEDS[sizes], nf=16)
    model = _model("argmax", nf=16)
    ref, S = _rev_ref(model, b, (sizes, 16, 32))
    with torch.no_grad():
        _, rev = model.reverse(_data(b), return_ldj=True)
    _within(f"rev_ldj {sizes} nf 16", rev.cpu().numpy(), ref, S)


# ---------------------------------------------------------------------------
# 2. hidden 128, f16x3, on every instance of the <= 32-atom kernel
# ---------------------------------------------------------------------------
_INSTANCE_LDJ = {}


def test_reverse_ldj_every_instance_h128(kernel_instance):
    sizes = (22, 32, 5, 1, 22, 17, 32, 2)
    b = _batch(sizes, 31)
    model = _model("argmax", hid=128, seed=32)
    ref, S = _rev_ref(model, b, (sizes, 5, 128))
    from enflow_amd import _lib
    with torch.no_grad():
        plain = model.reverse(_data(b))
        r0, m0 = _lib.FP32_RERUNS[0], _lib.FP32_MOL_RERUNS[0]
        out, rev = model.reverse(_data(b), return_ldj=True)
    whole_rerun = _lib.FP32_RERUNS[0] > r0 and _lib.FP32_MOL_RERUNS[0] == m0
    for k in ("h", "g", "pos", "vel"):      # the RLDJ instance of this kernel leaves the data bitwise the plain one's
        assert torch.equal(getattr(out, k), getattr(plain, k)), (kernel_instance, k)
    got = rev.cpu().numpy()
    _within(f"[{kernel_instance}] rev_ldj H=128", got, ref, S)
    for other, v in _INSTANCE_LDJ.items():
        nw = normwise(got, v)
        print(f"[{kernel_instance}] vs [{other}]: normwise {nw:.2e}")
        assert nw <= 1e-6, (kernel_instance, other, nw)
    _INSTANCE_LDJ[kernel_instance] = got
    # the same launch on caller buffers with the in-launch batch total (ldj_total + ticket)
    s = model._state(_data(b))
    n, M = s["h"].shape[0], len(sizes)
    idx = torch.empty(n, dtype=torch.int32, device=DEV)
    words = torch.zeros(3, dtype=torch.int32, device=DEV)      # error word, index maximum, ticket
    mol_err = torch.zeros(M, dtype=torch.int32, device=DEV)
    ldj_mol, total = torch.empty(M, device=DEV), torch.full((1,), float("nan"), device=DEV)
    with torch.no_grad():
        model.reverse_buffers(s["h"], s["g"], s["pos"], s["vel"], s["box"], s["r_cut"], s["mol_ptr"], s["max_n"],
                              idx, words[1:2], words[:1], src=s["src"], mol_err=mol_err, ldj_mol=ldj_mol,
                              ldj_total=total, ticket=words[2:])
    assert not int(words[0]) & ~_lib.ERR_RERUN and int(words[2]) == 0     # the ticket is reset
    # bitwise the module call's values, for every molecule this f16x3 launch did not flag (the
    # module call re-ran the flagged ones with fp32 GEMMs); most of the batch must be compared
    same = mol_err == 0
    print(f"[{kernel_instance}] reverse_buffers vs module call: {int(same.sum())} of {M} molecules compared bitwise "
          f"(error word {int(words[0])})")
    assert not whole_rerun, "the module call re-ran the whole batch in fp32: nothing to compare bitwise"
    assert int(same.sum()) >= M - M // 4
    assert torch.equal(ldj_mol[same], rev[same])
    want = float(ldj_mol.double().sum())
    assert abs(float(total) - want) <= 1e-6 * abs(want), (float(total), want)


# ---------------------------------------------------------------------------
# 3. return_ldj does not disturb the data; runs are bitwise reproducible
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(1, 2, 22, 32), (33, 64), (257, 3)])
def test_return_ldj_leaves_data_bitwise(sizes):
    b = _batch(sizes, SEEDS[sizes])
    model = _model("argmax")
    with torch.no_grad():
        plain = model.reverse(_data(b))
        out, rev = model.reverse(_data(b), return_ldj=True)
        _, rev2 = model.reverse(_data(b), return_ldj=True)
    for k in ("h", "g", "pos", "vel"):
        assert torch.equal(getattr(out, k), getattr(plain, k)), k
    assert torch.equal(rev, rev2)


# ---------------------------------------------------------------------------
# 4. forward(per_molecule=True)
# ---------------------------------------------------------------------------
def _fwd_ref(model, b, noise, kind, key, scale=1.0):
    """Per molecule: the oracle's one-molecule lf_forward value and S_m (cached)."""
    if key in _REV_REF:
        return _REV_REF[key]
    M = len(b["mol_ptr"]) - 1
    ref, S, r32 = np.zeros(M), np.zeros(M), np.zeros(M)
    okind = "argmax" if kind == "argmax" else "floor"
    for m in range(M):
        st1, n1 = _one(b, m, noise)
        dq = _dq(model) if kind == "argmax" else (scale if kind == "floor" else 0.0)
        _, ref[m] = O.lf_forward(_layers(model), dq, st1, n1 if kind != "none" else np.zeros_like(st1["h"]),
                                 model.dt, dequant_kind=okind)
        v, S[m] = fwd_one_restated(_layers(model), _dq(model) if kind == "argmax" else None, st1, n1, model.dt, kind,
                                   scale=scale)
        assert v == ref[m], "the forward restatement differs from lf_forward"
        r32[m], _ = fwd_one_restated(_layers(model, np.float32), _dq(model, np.float32) if kind == "argmax" else None,
                                     st1, n1, np.float32(model.dt), kind, np.float32, scale=scale)
    _floor_ok(f"forward {key}", r32, ref, S)
    _REV_REF[key] = (ref, S)
    return ref, S


@pytest.mark.parametrize("sizes", [(1, 2, 22, 32), (33, 64), (257, 3)])
def test_forward_per_molecule(sizes):
    b = _batch(sizes, SEEDS[sizes])
    M = len(sizes)
    model = _model("argmax")
    noise = torch.randn(b["h"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(41))
    ref, S = _fwd_ref(model, b, noise.cpu().double().numpy(), "argmax", ("fwd", sizes))
    with torch.no_grad():
        plain, scalar = model(_data(b), noise=noise)
        out, ldj_mol = model(_data(b), noise=noise, per_molecule=True)
        again = model(_data(b), noise=noise, per_molecule=True)[1]
    assert torch.equal(again, ldj_mol) and again.data_ptr() != ldj_mol.data_ptr()      # fresh tensors, not a view
    assert ldj_mol.shape == (M,) and ldj_mol.dtype == torch.float32
    for k in ("h", "g", "pos", "vel"):
        assert torch.equal(getattr(out, k), getattr(plain, k)), k
    # a molecule alone carries log_gaussian's whole -log(2 pi) / 2; in a batch the one
    # constant is shared equally (the documented split, so that the elements sum to the scalar)
    share = -0.5 * L2PI / M
    want = ref + 0.5 * L2PI + share
    _within(f"forward per molecule {sizes}", ldj_mol.cpu().numpy(), want, S + abs(share))
    tot, sc = float(ldj_mol.double().sum()), float(scalar)
    print(f"sum of elements {tot!r} vs scalar {sc!r}")
    assert abs(tot - sc) <= 1e-6 * abs(sc)


# ---------------------------------------------------------------------------
# 5. round trip
# ---------------------------------------------------------------------------
def test_round_trip_no_dequantiser():
    sizes = (1, 2, 22, 32)
    b = _batch(sizes, SEEDS[sizes])
    model = _model("none")
    _, S = _rev_ref(model, b, (sizes, 5, 32))
    with torch.no_grad():
        out, rev = model.reverse(_data(b), return_ldj=True)
        _, fwd = model(out, per_molecule=True)
    _within("round trip: forward(reverse(x)) vs -rev_ldj", fwd.cpu().numpy(), -rev.cpu().numpy(), S)


# ---------------------------------------------------------------------------
# 6. the per-molecule fp32 re-run
# ---------------------------------------------------------------------------
def test_per_molecule_fp32_rerun():
    """tests/test_gpu_small.py's construction: one molecule of an 8 x 22 batch at
    1e-4 magnitude (features 1e-4, geometry 1e-3) flags ENFLOW_ERR_SMALL in f16x3
    and is re-run alone with fp32 GEMMs; every molecule's values match the oracle."""
    from enflow_amd import _lib
    k, scale = 5, 1e-4
    base = dict(_batch((22,) * 8, 51))
    rng = np.random.default_rng(52)
    small = {kk: (v.copy() if isinstance(v, np.ndarray) else v) for kk, v in base.items()}
    small["h"] = np.floor(rng.uniform(0, 3, size=base["h"].shape))
    a0, a1 = int(base["mol_ptr"][k]), int(base["mol_ptr"][k + 1])
    for key, f in (("h", 1e-4), ("g", 1e-4), ("pos", 1e-3), ("vel", 1e-3), ("box", 1e-3)):
        small[key][a0:a1] = small[key][a0:a1] * f
    small["r_cut"][k] = small["r_cut"][k] * 1e-3
    small = _f32(small)
    model = _model("floor", seed=53, scale=scale)
    u = torch.rand(small["h"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(54))
    fref, fS = _fwd_ref(model, small, u.cpu().double().numpy(), "floor", ("fwd-small",), scale=scale)
    m0 = _lib.FP32_MOL_RERUNS[0]
    with torch.no_grad():
        out, fwd = model(_data(small), noise=u, per_molecule=True)
    assert _lib.FP32_MOL_RERUNS[0] - m0 == 1, "the forward re-ran other than the one flagged molecule"
    _within("forward per molecule with one fp32 re-run", fwd.cpu().numpy(), fref, fS)
    st = _state_of(out, small)
    rref, rS = _rev_ref(model, st, ("rev-small",))
    m0 = _lib.FP32_MOL_RERUNS[0]
    with torch.no_grad():
        _, rev = model.reverse(out, return_ldj=True)
    assert _lib.FP32_MOL_RERUNS[0] - m0 == 1, "the reverse re-ran other than the one flagged molecule"
    _within("rev_ldj with one fp32 re-run", rev.cpu().numpy(), rref, rS)


# ---------------------------------------------------------------------------
# 7. Alchemical_NLL.per_molecule / .potential
# ---------------------------------------------------------------------------
def _lj_abs(pos, softening):
    """Sum over i < j pairs of |4 r^-12| + |4 r^-6| (the terms lj_potential sums)."""
    d2 = np.triu(np.sum((pos[:, None, :] - pos[None, :, :]) ** 2, axis=2))
    r6 = (d2[d2 != 0] + softening) ** 3
    return float(np.sum(4.0 / r6 ** 2 + 4.0 / r6))


@pytest.mark.parametrize("softening", [0.0, 0.1])
def test_nll_per_molecule_and_potential(softening):
    from enflow_amd.flow import Alchemical_NLL
    from enflow_amd.data.synthetic import default_kBT
    sizes = (1, 2, 22, 65)
    b = _batch(sizes, 61)
    M, kBT, pf = len(sizes), default_kBT(), 10.0
    ldj = np.random.default_rng(62).normal(scale=20.0, size=M).astype(np.float32).astype(np.float64)
    pot, potS, nll, nllS, pot32, nll32 = (np.zeros(M) for _ in range(6))
    for m in range(M):
        s1 = _one(b, m)
        n = s1["pos"].shape[0]
        pot[m] = O.lj_potential(s1["pos"], s1["mol_ptr"], softening)
        nll[m] = O.alchemical_nll(s1, ldj[m], kBT, softening, pf)
        potS[m] = max(_lj_abs(s1["pos"], softening), 1e-30)
        logZ = -n * (math.log(pf) - 1.5 * math.log(2 * math.pi / kBT))
        nllS[m] = (potS[m] + 0.5 * np.sum(s1["vel"] ** 2)) / kBT + abs(logZ) + abs(ldj[m]) + \
            0.5 * np.sum(s1["h"] ** 2) + 0.5 * np.sum(s1["g"] ** 2) + L2PI
        s32 = _cast(s1, np.float32)
        pot32[m] = O.lj_potential(s32["pos"], s32["mol_ptr"], np.float32(softening))
        nll32[m] = O.alchemical_nll(s32, np.float32(ldj[m]), np.float32(kBT), np.float32(softening), pf)
    keep = potS > 1e-30      # (the one-atom molecule has no pairs: its energy is exactly zero)
    _floor_ok(f"lj_potential softening {softening}", pot32[keep], pot[keep], potS[keep])
    _floor_ok(f"alchemical_nll softening {softening}", nll32, nll, nllS)
    loss = Alchemical_NLL(kBT=kBT, partition_func=pf, softening=softening)
    d = _data(b)
    ldj_t = torch.tensor(ldj, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        got_pot = loss.potential(d)
        got = loss.per_molecule(d, ldj_t)
        scalar = loss(d, ldj_t.double().sum().float())
    assert got_pot.shape == (M,) and got.shape == (M,)
    assert float(got_pot[0]) == 0.0
    _within(f"potential softening {softening}", got_pot.cpu().numpy()[keep], pot[keep], potS[keep])
    _within(f"per_molecule softening {softening}", got.cpu().numpy(), nll, nllS)
    # per_molecule.mean() - nll(out, ldj_mol.sum()) = (M - 1) / M * log(2 pi); both sides are fp32
    # values of terms summing to at most mean(S_m), so the identity holds to 1e-5 of that
    lhs = float(got.double().mean()) - float(scalar)
    rhs = (M - 1) / M * L2PI
    print(f"identity: {lhs!r} vs {rhs!r} (scale {float(np.mean(nllS)):.3e})")
    assert abs(lhs - rhs) <= TOL * float(np.mean(nllS))
