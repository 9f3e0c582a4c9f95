"""Cooperative leftover pair tiles (enflow_set_coop_tiles) of the 4-wave
<= 32-atom hidden_nf = 128 f16x3 flow instance: a layer whose unique pairs make
T = 4 q + r tiles of 32 with r = 1 or 2 runs the last r tiles on the four waves
together (flow_device.h, edge_tiles, COOP).

Geometry: molecules whose atoms all lie within r_cut of each other in a box
far wider than r_cut have exactly n (n - 1) unique pairs, so the atom count
picks T and T mod 4; the oracle's pair count of every molecule and layer input
is asserted first, so a geometry that drifts fails instead of passing
vacuously.  Bars: the project's 1e-5 normwise per tensor against the float64
oracle (enflow/flow/dynamics.py:10-37), 1e-5 relative on log|detJ|; the
on-versus-off difference of a molecule is bounded by its own errors against
the oracle; everything said to be unchanged is compared bitwise."""
import numpy as np
import pytest
import torch

from oracle import enflow_oracle as O
from _fixtures import normwise, scalar_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
RC = 2   # COOP_RC of flow_device.h: most leftover tiles run cooperatively
KEYS = ("h", "g", "pos", "vel")

# name -> (atom counts, make_molecules keywords, hidden_nf)
FULL = dict(r_cut_ang=20.0, box_ang=100.0)   # every other atom within r_cut, no image in reach
CASES = {
    "full_a": ([16, 17, 18, 19, 31], FULL, 128),
    "full_b": ([12, 14, 26, 2, 1], FULL, 128),
    "default22": ([22] * 6, {}, 128),
    "box5": ([22] * 4, dict(box_ang=5.0), 128),
    "h32": ([17, 18, 16], FULL, 32),
}


@pytest.fixture(scope="module", autouse=True)
def _four_wave_instance():
    """The 4-wave whole-tile instance for every launch of this file (a small
    batch otherwise goes to the 8-wave or the feature-split instances)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from enflow_amd import _lib
    prev = (_lib.set_latency_threshold(0), _lib.set_split_threshold(0), _lib.set_fs_threshold(0))
    yield
    _lib.set_latency_threshold(-1 if prev[0] is None else prev[0])
    _lib.set_split_threshold(-1 if prev[1] is None else prev[1])
    _lib.set_fs_threshold(-1 if prev[2] is None else prev[2])


class _coop:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from enflow_amd import _lib
        self.prev = _lib.set_coop_tiles(self.on)

    def __exit__(self, *exc):
        from enflow_amd import _lib
        _lib.set_coop_tiles(True if self.prev is None else self.prev)
        return False


class _order:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from enflow_amd import _lib
        self.prev = _lib.set_longest_first(self.mode)

    def __exit__(self, *exc):
        from enflow_amd import _lib
        _lib.set_longest_first(1 if self.prev is None else self.prev)
        return False


def _f32(b):
    out = dict(b)
    for k in ("h", "g", "pos", "vel", "box", "r_cut"):
        out[k] = np.asarray(b[k], dtype=np.float32).astype(np.float64)
    return out


def _batch(sizes, seed, **kw):
    from enflow_amd.data.synthetic import make_molecules
    return _f32(make_molecules(len(sizes), list(sizes), nf=5, seed=seed, **kw))


def _model(hid, seed, scale=1.0):
    from enflow_amd.nn import EGCL, Floor
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    torch.manual_seed(seed)
    m = LFIntegrator([EGCL(5, 5, hid) for _ in range(2)], Floor(dequant_scale=scale), dt=default_dt()).to(DEV)
    m.gemm_precision = "f16x3"
    return m


def _layers(model):
    out = []
    for n in model.networks:
        p = {k: v.detach().cpu().double().numpy() for k, v in n.state_dict().items()}
        p["flags"] = (False, False, False)
        out.append(p)
    return out


def _mol(b, m):
    a0, a1 = int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1])
    s = {k: b[k][a0:a1] for k in KEYS + ("box",)}
    s.update(r_cut=b["r_cut"][m:m + 1], mol_ptr=np.array([0, a1 - a0], dtype=np.int64))
    return s


def _pairs(s):
    """Unique (row, col) pairs of one molecule at the state's positions."""
    row, col, _ = O.batch_edges(s["pos"], s["box"], s["r_cut"], s["mol_ptr"])
    return len(O.pair_multiplicity(row, col, max(len(s["pos"]), 1))[0])


def _oracle_forward(model, b, u):
    """Per molecule: the float64 forward, log|detJ| and the unique pairs at every
    layer's input (dynamics.py:10-24 one layer at a time)."""
    layers, scale, dt = _layers(model), float(model.dequantize.dequant_scale), model.dt
    un = u.cpu().double().numpy()
    ref = {k: [] for k in KEYS}
    ldj, counts = [], []
    for m in range(len(b["mol_ptr"]) - 1):
        a0, a1 = int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1])
        s = {k: np.array(v, copy=True) for k, v in _mol(b, m).items()}
        s["h"], l = O.floor_forward(s["h"], un[a0:a1], scale)
        cm = []
        for p in layers:
            cm.append(_pairs(s))
            s, dl = O.lf_forward([p], 0.0, s, np.zeros_like(s["h"]), dt, dequant_kind="floor")
            l += dl
        for k in KEYS:
            ref[k].append(s[k])
        ldj.append(l)
        counts.append(cm)
    return {k: np.concatenate(v) for k, v in ref.items()}, np.array(ldj), np.array(counts)


def _oracle_reverse(model, b, state):
    """Per molecule: the float64 reverse of `state` (the continuous h, before the
    dequantiser's floor) and the unique pairs at every layer's input."""
    layers, dt = _layers(model), model.dt
    ref = {k: [] for k in KEYS}
    counts = []
    full = dict(b)
    full.update({k: np.asarray(state[k], dtype=np.float64) for k in KEYS})
    for m in range(len(b["mol_ptr"]) - 1):
        s = {k: np.array(v, copy=True) for k, v in _mol(full, m).items()}
        cm = []
        for p in reversed(layers):
            probe = dict(s)
            probe["pos"] = O.apply_pbc(s["pos"] - s["vel"] * dt, s["box"])
            cm.append(_pairs(probe))
            s = O.lf_reverse([p], s, dt, dequant_kind="none")
        for k in KEYS:
            ref[k].append(s[k])
        counts.append(cm)
    return {k: np.concatenate(v) for k, v in ref.items()}, np.array(counts)


def _forward(model, b, u, on, order=1):
    """One raw forward launch (no host retry) with the switch `on`."""
    from enflow_amd import _lib
    from enflow_amd.data import Data
    s = model._state(Data.from_arrays(b, device=DEV))
    M = s["mol_ptr"].numel() - 1
    ldj_mol, ldj = torch.zeros(max(M, 1), device=DEV), torch.zeros(1, device=DEV)
    st = torch.zeros(2, dtype=torch.int32, device=DEV)
    with _coop(on), _order(order), _lib.KernelTimer() as t, torch.no_grad():
        model.forward_buffers(s["h"], s["g"], s["pos"], s["vel"], s["box"], s["r_cut"], s["mol_ptr"], s["max_n"],
                              u, ldj_mol, ldj, st[:1], src=s["src"], ticket=st[1:])
    torch.cuda.synchronize()
    out = {k: s[k].clone() for k in KEYS}
    out.update(ldj_mol=ldj_mol, ldj=ldj, err=st[:1].clone())
    return out, set(t.stats)


def _reverse(model, b, state, on, order=1):
    from enflow_amd import _lib
    from enflow_amd.data import Data
    s = model._state(Data.from_arrays(b, device=DEV))
    src = tuple(state[k] for k in KEYS)
    idx = torch.zeros(max(src[0].shape[0], 1), dtype=torch.int32, device=DEV)
    rv = torch.zeros(2, dtype=torch.int32, device=DEV)
    with _coop(on), _order(order), _lib.KernelTimer() as t, torch.no_grad():
        model.reverse_buffers(s["h"], s["g"], s["pos"], s["vel"], s["box"], s["r_cut"], s["mol_ptr"], s["max_n"],
                              idx, rv[1:], rv[:1], src=src)
    torch.cuda.synchronize()
    out = {k: s[k].clone() for k in ("g", "pos", "vel")}   # h: floor() of the continuous value (not compared)
    out.update(err=rv[:1].clone())
    return out, set(t.stats)


def _has_coop(counts):
    """Per molecule: does any layer have 1 .. RC leftover tiles?"""
    r = ((counts + 31) // 32) % 4
    return ((r > 0) & (r <= RC)).any(axis=1)


def _same(a, b, what, rows=None):
    for k in a:
        x, y = a[k], b[k]
        if rows is not None and x.shape[0] == rows.shape[0]:
            x, y = x[rows], y[rows]
        assert torch.equal(x, y), f"{what}: {k} differs"


def _mol_errs(out, ref, b, keys, extra=None):
    """Per molecule: the largest normwise error over `keys` (and |extra| pairs)."""
    errs = []
    for m in range(len(b["mol_ptr"]) - 1):
        a0, a1 = int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1])
        e = [normwise(np.asarray(out[k])[a0:a1], np.asarray(ref[k])[a0:a1]) for k in keys if a1 > a0]
        if extra is not None:
            e.append(scalar_rel(extra[0][m], extra[1][m]) if extra[1][m] != 0 else abs(float(extra[0][m])))
        errs.append(max(e) if e else 0.0)
    return np.array(errs)


_cache = {}


def _run(name):
    """Forward and reverse of a case with the switch on and off, and the oracle's
    results, computed once and shared (never modified)."""
    if name in _cache:
        return _cache[name]
    sizes, kw, hid = CASES[name]
    b = _batch(sizes, 90 + len(_cache), **kw)
    model = _model(hid, 91)
    u = torch.rand(b["h"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(92))
    ref, ref_ldj, counts = _oracle_forward(model, b, u)
    f_on, kern = _forward(model, b, u, True)
    f_off, _ = _forward(model, b, u, False)
    assert any(k.startswith("lf_flow_kernel") for k in kern), kern
    rref, rcounts = _oracle_reverse(model, b, {k: f_off[k].cpu().numpy() for k in KEYS})
    r_on, _ = _reverse(model, b, f_off, True)
    r_off, _ = _reverse(model, b, f_off, False)
    res = dict(b=b, model=model, u=u, ref=ref, ref_ldj=ref_ldj, counts=counts, rref=rref, rcounts=rcounts,
               f_on=f_on, f_off=f_off, r_on=r_on, r_off=r_off, hid=hid)
    print(f"{name}: atoms {sizes}, unique pairs per layer input forward {counts.tolist()} reverse {rcounts.tolist()}")
    _cache[name] = res
    return res


def test_pair_counts_and_remainder_coverage():
    """The all-within-r_cut molecules have n (n - 1) unique pairs at the first
    layer's input (oracle), the listed tile counts, and every T mod 4 occurs."""
    want_T = {16: 8, 17: 9, 18: 10, 19: 11, 31: 30, 12: 5, 14: 6, 26: 21, 2: 1, 1: 0}
    seen = set()
    for name in ("full_a", "full_b", "h32"):
        r = _run(name)
        for n, c in zip(CASES[name][0], r["counts"][:, 0]):
            assert c == n * (n - 1), (name, n, c)
            assert (c + 31) // 32 == want_T[n]
            if c:
                seen.add(int((c + 31) // 32) % 4)
    assert seen == {0, 1, 2, 3}, seen
    # the narrowest tail: the last cooperative tile of 31 atoms holds 2 valid pairs
    assert 31 * 30 - 29 * 32 == 2
    for name in ("default22", "box5"):
        r = _run(name)
        print(name, "tiles mod 4 per layer:", (((r["counts"] + 31) // 32) % 4).tolist())
    assert _has_coop(_run("default22")["counts"]).any() or _has_coop(_run("box5")["counts"]).any()


@pytest.mark.parametrize("name", list(CASES))
def test_switch_on_matches_the_oracle(name):
    """Forward and reverse with the switch on: 1e-5 normwise per tensor, 1e-5
    relative on log|detJ| (batch and per molecule), error word zero."""
    r = _run(name)
    b, f, rv = r["b"], r["f_on"], r["r_on"]
    errs = {k: normwise(f[k].cpu().numpy(), r["ref"][k]) for k in KEYS}
    errs["ldj"] = scalar_rel(float(f["ldj"]), float(np.sum(r["ref_ldj"])))
    lm = f["ldj_mol"].cpu().numpy()
    for m, want in enumerate(r["ref_ldj"]):
        errs[f"ldj_mol{m}"] = scalar_rel(lm[m], want) if want != 0 else abs(float(lm[m]))
    rerrs = {"rev_" + k: normwise(rv[k].cpu().numpy(), r["rref"][k]) for k in ("g", "pos", "vel")}
    print(name, {k: f"{v:.2e}" for k, v in {**errs, **rerrs}.items()})
    assert int(f["err"]) == 0 and int(rv["err"]) == 0
    bad = {k: v for k, v in {**errs, **rerrs}.items() if not (np.isfinite(v) and v <= TOL)}
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_switch_on_against_off(name):
    """Molecules without a cooperative tile in any layer: every output and the
    per-molecule log|detJ| bitwise equal with the switch on and off (H = 32: all
    of them).  The others: the on/off difference, printed, is no larger than
    the molecule's larger error against the oracle."""
    r = _run(name)
    b = r["b"]
    atom_mol = np.repeat(np.arange(len(b["mol_ptr"]) - 1), np.diff(b["mol_ptr"]))
    for what, on, off, ref, counts, keys, extra in (
            ("forward", r["f_on"], r["f_off"], r["ref"], r["counts"], KEYS, True),
            ("reverse", r["r_on"], r["r_off"], r["rref"], r["rcounts"], ("g", "pos", "vel"), False)):
        coop = _has_coop(counts) if r["hid"] == 128 else np.zeros(len(counts), dtype=bool)
        keep = torch.as_tensor(~coop[atom_mol], device=DEV)
        for k in keys:
            assert torch.equal(on[k][keep], off[k][keep]), f"{name} {what}: {k} of an untouched molecule moved"
        if extra:
            km = torch.as_tensor(~coop, device=DEV)
            assert torch.equal(on["ldj_mol"][km], off["ldj_mol"][km]), f"{name}: log|detJ| of an untouched molecule"
        assert torch.equal(on["err"], off["err"])
        onc = {k: on[k].cpu().numpy() for k in keys}
        offc = {k: off[k].cpu().numpy() for k in keys}
        ex = (lambda o: (o["ldj_mol"].cpu().numpy(), r["ref_ldj"])) if extra else (lambda o: None)
        e_on, e_off = _mol_errs(onc, ref, b, keys, ex(on)), _mol_errs(offc, ref, b, keys, ex(off))
        dex = (on["ldj_mol"].cpu().numpy(), off["ldj_mol"].cpu().numpy()) if extra else None
        d = _mol_errs(onc, offc, b, keys, dex)
        print(f"{name} {what}: cooperative {coop.tolist()} on/off {[f'{x:.1e}' for x in d]} "
              f"on/oracle {[f'{x:.1e}' for x in e_on]} off/oracle {[f'{x:.1e}' for x in e_off]}")
        for m in np.nonzero(coop)[0]:
            assert d[m] <= max(e_on[m], e_off[m]), (name, what, int(m), d[m], e_on[m], e_off[m])


@pytest.mark.parametrize("name", ["full_a", "default22"])
def test_reproducible_and_order_independent(name):
    """Two launches with the switch on are bitwise equal; so are longest-first
    always (2) and batch order (0) with the switch on."""
    r = _run(name)
    again, _ = _forward(r["model"], r["b"], r["u"], True)
    _same(again, r["f_on"], f"{name}: second run")
    f2, k2 = _forward(r["model"], r["b"], r["u"], True, order=2)
    f0, k0 = _forward(r["model"], r["b"], r["u"], True, order=0)
    assert "order_key_kernel" in k2 and "order_key_kernel" not in k0
    _same(f2, f0, f"{name}: longest-first vs batch order")
    _same(f2, r["f_on"], f"{name}: order 2 vs auto")
    v2, _ = _reverse(r["model"], r["b"], r["f_off"], True, order=2)
    _same(v2, r["r_on"], f"{name}: reverse, order 2 vs auto")


def test_other_instances_ignore_the_switch():
    """The 8-wave instance (set_latency_threshold) and a 33-atom molecule on the
    64-atom image: bitwise equal with the switch on and off."""
    from enflow_amd import _lib
    r = _run("full_a")
    prev = _lib.set_latency_threshold(1 << 30)
    try:
        a, ka = _forward(r["model"], r["b"], r["u"], True)
        c, _ = _forward(r["model"], r["b"], r["u"], False)
        ra, _ = _reverse(r["model"], r["b"], r["f_off"], True)
        rc, _ = _reverse(r["model"], r["b"], r["f_off"], False)
    finally:
        _lib.set_latency_threshold(0 if prev is None else prev)
    _same(a, c, "8-wave forward")
    _same(ra, rc, "8-wave reverse")
    b = _batch([33, 17, 18], 95, **FULL)
    u = torch.rand(b["h"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(96))
    a, _ = _forward(r["model"], b, u, True)
    c, _ = _forward(r["model"], b, u, False)
    _same(a, c, "64-atom image forward")
    ra, _ = _reverse(r["model"], b, c, True)
    rc, _ = _reverse(r["model"], b, c, False)
    _same(ra, rc, "64-atom image reverse")
    assert int(a["err"]) == 0


def test_small_operand_guard_fires_on_cooperative_tiles():
    """tests/test_gpu_small.py's construction (h, g ~1e-3, layer 1's edge_nn.0
    scaled by 1e-3) on molecules with one and two cooperative tiles: the raw
    launch sets the same error bits with the switch on as off
    (ENFLOW_ERR_SMALL), and the module call's fp32 re-run meets the bar."""
    from enflow_amd import _lib
    from enflow_amd.data import Data
    scale = 1e-3
    b = _batch([17, 18, 16], 97, **FULL)
    rng = np.random.default_rng(98)
    b["h"] = _f32({**b, "h": np.floor(rng.uniform(0, 3, size=b["h"].shape)) * scale})["h"]
    b["g"] = _f32({**b, "g": b["g"] * scale})["g"]
    model = _model(128, 99, scale)
    with torch.no_grad():
        lin = model.networks[1].edge_nn[0]
        lin.weight.mul_(scale)
        lin.bias.mul_(scale)
    model._layers_key = None
    u = torch.rand(b["h"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(100))
    ref, ref_ldj, counts = _oracle_forward(model, b, u)
    assert _has_coop(counts)[:2].all(), counts
    on, _ = _forward(model, b, u, True)
    off, _ = _forward(model, b, u, False)
    print("raw error words on / off:", int(on["err"]), int(off["err"]))
    assert int(on["err"]) == int(off["err"]) and int(on["err"]) & _lib.ERR_SMALL
    n0 = _lib.FP32_RERUNS[0]
    with _coop(True), torch.no_grad():
        o, ldj = model(Data.from_arrays(b, device=DEV), noise=u)
    assert _lib.FP32_RERUNS[0] - n0 == 1
    errs = {k: normwise(getattr(o, k).cpu().numpy(), ref[k]) for k in KEYS}
    errs["ldj"] = scalar_rel(float(ldj.sum()), float(np.sum(ref_ldj)))
    print("fp32 re-run vs oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(np.isfinite(v) and v <= TOL for v in errs.values()), errs
