"""The HIP training backward (enflow_amd/csrc/enflow_backward.hip) at the batch
layouts where tile code breaks, and the gradients it returns for the data.

* input gradients -- d loss / d g, pos, vel of the data (d h under Floor) --
  against the reference's own loss.backward() (goldens train_in_* of
  tests/golden/make_golden.py train_inputs);
* edge layouts against the float64 gradient oracle (pinned to those goldens):
  1- and 2-atom molecules, rows without pairs, a batch without any pair,
  periodic multiplicities above 1, the 32/33 and 64/65 size boundaries;
* upstream adjoints other than the NLL's (some of them None, a loss scale);
* enflow_alchemical_nll_backward_f32 on its own.

Bars: GRAD_TOL normwise per tensor, LOSS_TOL on the loss (tests/test_gpu_train.py).
They stay a real test only where float32 rounding alone sits well inside
them, so every case also asserts, on the CPU, that the oracle run in float32
is within half the bar of the float64 oracle, for every tensor it compares.
A tensor whose oracle gradient is exactly zero must be exactly zero on the GPU.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import enflow_oracle as O
from oracle import enflow_oracle_grad as OG
from _fixtures import (load, flow_from_fixture, egcl_from_fixture, state, n_layers, normwise, scalar_rel, worst_of,
                       assert_all_within)
from test_gpu_train import GRAD_TOL, LOSS_TOL

pytestmark = pytest.mark.gpu

NL = 2
LIBS = {"h64nf5": (64, 5), "h32nf16": (32, 16)}    # the 8-feature library; the 16-feature one (radial row: wrad)
# id -> (sizes, make_molecules keywords, data seed)
CASES = {
    "tiny": ([1, 2, 22, 5], {}, 7),
    "bound32": ([32, 31, 1], {}, 7),
    "bound64": ([33, 64, 2], dict(radius=5.7), 7),
    "large65": ([65, 1, 22], dict(radius=5.7), 7),
    # the walk's bonds (1.5 A) are inside this cut-off, so an atom without any edge is rare:
    # seed 7 has none, 14 has one in the nf 5 and one in the nf 16 draw
    "sparse": ([22, 31, 9, 17, 2], dict(r_cut_ang=1.6), 14),
    "mult": ([22, 31, 9, 2], dict(r_cut_ang=3.0, box_ang=5.0), 7),
    # seed 7 leaves one edge in the nf 16 draw; 22 is the first seed with none in either
    "nopairs": ([1, 1, 2, 3], dict(r_cut_ang=0.5), 22),
}
F32_TOO = ("mult", "bound64", "large65")           # also with gemm_precision "f32" (the ENFLOW_BWD_F32 backward)
EDGE_PARAMS = [(c, l, p) for c in CASES for l in LIBS for p in (("f16x3", "f32") if c in F32_TOO else ("f16x3",))]


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _setup(case, lib):
    """The case's batch (float32-representable), noise, the CPU model (weights
    from torch.manual_seed(3)) and its parameters as float64 numpy; the layout
    the case is there for is checked here, on the CPU."""
    from enflow_amd import _lib
    from enflow_amd.data.synthetic import make_molecules, default_dt
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    sizes, kw, seed = CASES[case]
    hid, nf = LIBS[lib]
    b = make_molecules(len(sizes), sizes, nf=nf, seed=seed, **kw)
    for k in ("h", "g", "pos", "vel", "box", "r_cut"):
        b[k] = _f32(b[k])
    _pin_layout(case, b, _lib.TRAIN_MAX_ATOMS)
    torch.manual_seed(3)
    model = LFIntegrator([EGCL(nf, nf, hid) for _ in range(NL)], ArgMax(nf, hid), dt=default_dt())
    eps = np.random.default_rng(13).normal(size=b["h"].shape).astype(np.float32)
    layers = [{k: v.detach().double().numpy() for k, v in n.named_parameters()} for n in model.networks]
    dq = {k: v.detach().double().numpy() for k, v in model.dequantize.named_parameters()}
    return dict(b=b, eps=eps, model=model, layers=layers, dq=dq, dt=default_dt())


def _pin_layout(case, b, train_max_atoms):
    """The layer-0 neighbour list has the property the case is named for."""
    ptr = b["mol_ptr"]
    n, max_n = int(ptr[-1]), int(np.diff(ptr).max())
    row, col, _ = O.batch_edges(b["pos"], b["box"], b["r_cut"], ptr)
    if case == "nopairs":
        assert len(row) == 0
    else:
        assert len(row) > 0
    if case == "mult":
        assert int(O.pair_multiplicity(row, col, n)[2].max()) >= 2
    if case == "sparse":
        assert len(set(range(n)) - set(row.tolist())) >= 1
    if case == "tiny":
        assert ptr[1] == 1 and 0 not in row and 0 not in col
    if case == "large65":
        assert max_n > train_max_atoms
    if case == "bound64":
        assert max_n == 64 == train_max_atoms
    if case == "bound32":
        assert max_n == 32


def _flat(gl, gd, gi):
    out = {f"p{i}.{k}": v for i, g in enumerate(gl) for k, v in g.items()}
    out.update({f"dq.{k}": v for k, v in gd.items()})
    out.update({f"in.{k}": v for k, v in gi.items()})
    return out


def _assert_f32_floor(name, ref, ref32):
    """(loss, grads) of the float64 oracle and of the same oracle in float32:
    float32 rounding alone stays within half of each bar.  Returns the worst
    gradient floor."""
    floor = {k: normwise(ref32[1][k], v) for k, v in ref[1].items()}
    lfloor = scalar_rel(ref32[0], ref[0])
    assert lfloor <= LOSS_TOL / 2, f"{name}: the float32 oracle's loss is {lfloor:.2e} off the float64 one"
    assert_all_within(floor, GRAD_TOL / 2, f"{name}: float32 oracle vs float64 oracle")
    return worst_of(floor)


def _compare(name, loss, got, ref, floor):
    lerr = scalar_rel(loss, ref[0])
    assert sorted(got) == sorted(ref[1])
    errs = {k: normwise(got[k], v) for k, v in ref[1].items()}
    wk = max(errs, key=lambda k: (not np.isfinite(errs[k]), errs[k]))
    zeros = [k for k, v in ref[1].items() if not np.any(v)]
    fl = "" if floor is None else f", float32-oracle floor {floor:.2e}"
    print(f"{name}: loss err {lerr:.2e}, worst grad err {errs[wk]:.2e} ({wk}){fl}, {len(zeros)} all-zero tensors")
    assert lerr <= LOSS_TOL, (float(loss), ref[0])
    for k in zeros:
        assert not np.any(got[k]), f"{name}: {k} is exactly zero in the oracle, not on the GPU"
    assert_all_within(errs, GRAD_TOL, name)


def _gpu_batch(b, floor_h=False):
    """Data on the GPU whose g, pos, vel (and h) are leaves that require grad."""
    from enflow_amd.data import Data
    t = lambda k: torch.tensor(b[k], dtype=torch.float32, device="cuda")  # noqa: E731
    leaves = {k: t(k).requires_grad_(True) for k in (("h",) if floor_h else ()) + ("g", "pos", "vel")}
    data = Data(h=leaves.get("h", t("h")), g=leaves["g"], pos=leaves["pos"], vel=leaves["vel"],
                N=torch.tensor(np.diff(b["mol_ptr"])), r_cut=t("r_cut"), box=t("box"), device="cuda")
    return data, leaves


def _gpu_grads(model, leaves):
    torch.cuda.synchronize()
    got = {}
    for i, net in enumerate(model.networks):
        for k, p in net.named_parameters():
            assert p.grad is not None, f"layer {i} {k} has no gradient"
            got[f"p{i}.{k}"] = p.grad.double().cpu().numpy()
    if model.dequantize is not None:
        for k, p in model.dequantize.named_parameters():
            assert p.grad is not None, f"dequantiser {k} has no gradient"
            got[f"dq.{k}"] = p.grad.double().cpu().numpy()
    for k, v in leaves.items():
        assert v.grad is not None, f"the data's {k} has no gradient"
        got[f"in.{k}"] = v.grad.double().cpu().numpy()
    return got


# ---------------------------------------------------------------------------
# a. input gradients against the reference's loss.backward()
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["train_in_h32_L2", "train_floor_in_h32_L2"])
def test_input_gradients_match_reference(name):
    from enflow_amd.flow import Alchemical_NLL, LFIntegrator
    from enflow_amd.nn import Floor
    inp, ref = load(name)
    floor = "dequant_scale" in inp
    if floor:
        hid, nf = int(inp["hid"]), inp["h"].shape[1]
        model = LFIntegrator([egcl_from_fixture(inp, i, nf, hid) for i in range(n_layers(inp))],
                             Floor(float(inp["dequant_scale"])), dt=float(inp["dt"])).cuda()
    else:
        model, _ = flow_from_fixture(inp, "cuda")
    data, leaves = _gpu_batch(state(inp), floor_h=floor)
    out, ldj = model(data, noise=torch.tensor(inp["eps"], dtype=torch.float32, device="cuda"))
    loss = Alchemical_NLL(kBT=float(inp["kBT"]), softening=float(inp["softening"]))(out, ldj)
    loss.backward()
    got = _gpu_grads(model, leaves)
    want = {k[5:].replace("in_", "in."): v for k, v in ref.items() if k.startswith("grad_")}
    assert sorted(k for k in want if k.startswith("in.")) == sorted(f"in.{k}" for k in leaves)
    _compare(name, float(loss.detach()), got, (float(ref["loss"]), want), None)


# ---------------------------------------------------------------------------
# b. edge layouts against the oracle
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nll_ref(case, lib):
    """((loss, grads) float64, the float32-oracle floor) of one NLL training step."""
    from enflow_amd.data.synthetic import default_kBT
    s = _setup(case, lib)
    res = []
    for dtype in (torch.float64, torch.float32):
        loss, _, gl, gd, _, gi = OG.train_loss_and_grads(s["layers"], s["dq"], s["b"], s["eps"].astype(np.float64),
                                                         s["dt"], default_kBT(), 0.1, dtype=dtype, input_grads=True)
        res.append((loss, _flat(gl, gd, gi)))
    return res[0], _assert_f32_floor(f"{case}-{lib}", *res)


@pytest.mark.parametrize("case,lib,prec", EDGE_PARAMS, ids=["-".join(p) for p in EDGE_PARAMS])
def test_edge_layout_gradients_vs_oracle(case, lib, prec):
    from enflow_amd.flow import Alchemical_NLL
    from enflow_amd.data.synthetic import default_kBT
    s = _setup(case, lib)
    ref, floor = _nll_ref(case, lib)
    if case == "nopairs":      # no edge in either layer: the message networks get exact zeros
        zero = {k for k, v in ref[1].items() if not np.any(v)}
        assert {f"p{i}.{k}" for i in range(NL) for k in s["layers"][i] if k.startswith(("edge_nn.", "coord_nn."))} \
            <= zero, zero
    model = copy.deepcopy(s["model"]).cuda()
    model.gemm_precision = prec
    data, leaves = _gpu_batch(s["b"])
    out, ldj = model(data, noise=torch.tensor(s["eps"], device="cuda"))
    loss = Alchemical_NLL(kBT=default_kBT(), softening=0.1)(out, ldj)
    loss.backward()
    _compare(f"{case}-{lib}-{prec}", float(loss.detach()), _gpu_grads(model, leaves), ref, floor)


# ---------------------------------------------------------------------------
# c. upstream adjoints other than the NLL's
# ---------------------------------------------------------------------------
LOSSES = ("weighted", "ldj_only", "pos_only", "scaled_nll")


def _upstream_loss(kind, out, ldj, w, nll):
    """out: dict of h, g, pos, vel tensors; w: same-shaped fixed weights."""
    if kind == "weighted":
        return sum((w[k] * out[k]).sum() for k in ("h", "g", "pos", "vel")) + 0.7 * ldj
    if kind == "ldj_only":
        return ldj
    if kind == "pos_only":
        return (w["pos"] * out["pos"]).sum()
    return 0.37 * nll(out, ldj)


def _weights(b):
    rng = np.random.default_rng(29)
    return {k: rng.normal(size=b[k].shape).astype(np.float32) for k in ("h", "g", "pos", "vel")}


@functools.lru_cache(maxsize=None)
def _upstream_ref(case, lib, kind):
    from enflow_amd.data.synthetic import default_kBT
    s = _setup(case, lib)
    b = s["b"]
    res = []
    for dtype in (torch.float64, torch.float32):
        h, g, pos, vel, ldj, P, D, leaves = OG.flow_forward_torch(s["layers"], s["dq"], b, s["eps"].astype(np.float64),
                                                                  s["dt"], dtype=dtype, input_grads=True)
        w = {k: torch.tensor(v.astype(np.float64)).to(dtype) for k, v in _weights(b).items()}
        nll = lambda o, l: OG._nll(o["h"], o["g"], o["pos"], o["vel"], l, b["mol_ptr"], default_kBT(), 0.1, 10.0)  # noqa: E731,E741
        loss = _upstream_loss(kind, dict(h=h, g=g, pos=pos, vel=vel), ldj, w, nll)
        loss.backward()
        res.append((float(loss.detach()), _flat(*OG.collect_grads(P, D, leaves))))
    return res[0], _assert_f32_floor(f"{case}-{lib}-{kind}", *res)


@pytest.mark.parametrize("kind", LOSSES)
@pytest.mark.parametrize("case", ["bound32", "large65"])
def test_upstream_adjoints_vs_oracle(case, kind):
    from enflow_amd.flow import Alchemical_NLL
    from enflow_amd.data.synthetic import default_kBT
    lib = "h64nf5"
    s = _setup(case, lib)
    ref, floor = _upstream_ref(case, lib, kind)
    model = copy.deepcopy(s["model"]).cuda()
    data, leaves = _gpu_batch(s["b"])
    out, ldj = model(data, noise=torch.tensor(s["eps"], device="cuda"))
    w = {k: torch.tensor(v, device="cuda") for k, v in _weights(s["b"]).items()}
    od = dict(h=out.h, g=out.g, pos=out.pos, vel=out.vel)
    loss = _upstream_loss(kind, od, ldj, w, lambda o, l: Alchemical_NLL(kBT=default_kBT(), softening=0.1)(out, l))  # noqa: E741
    loss.backward()
    _compare(f"{case}-{kind}", float(loss.detach()), _gpu_grads(model, leaves), ref, floor)


# ---------------------------------------------------------------------------
# d. Alchemical_NLL alone
# ---------------------------------------------------------------------------
NLL_SIZES = [1, 2, 22, 65]     # no pair; one pair; one wave per molecule; past 64 atoms: one wave per atom


@functools.lru_cache(maxsize=None)
def _nll_alone(kBT, softening):
    from enflow_amd.data.synthetic import make_molecules
    b = make_molecules(len(NLL_SIZES), NLL_SIZES, nf=5, seed=7, radius=5.7)
    for k in ("h", "g", "pos", "vel"):
        b[k] = _f32(b[k])
    b["h"] = _f32(b["h"] + 0.25 * np.random.default_rng(17).normal(size=b["h"].shape))   # as after a flow, not one-hot
    ptr = b["mol_ptr"]
    if softening == 0:
        # one atom copied exactly onto another, in the 22- and in the 65-atom molecule:
        # the reference drops zero distances (loss.py:15), which needs bitwise-equal rows
        for m, (i, j) in ((2, (3, 17)), (3, (10, 60))):
            b["pos"][ptr[m] + j] = b["pos"][ptr[m] + i]
            assert np.array_equal(b["pos"][ptr[m] + i].astype(np.float32), b["pos"][ptr[m] + j].astype(np.float32))
    ldj = float(np.float32(-3.75))
    res = []
    for dtype in (torch.float64, torch.float32):
        lv = {k: torch.tensor(b[k]).to(dtype).requires_grad_(True) for k in ("h", "g", "pos", "vel")}
        lv["ldj"] = torch.tensor(ldj, dtype=dtype, requires_grad=True)
        loss = 0.37 * OG._nll(lv["h"], lv["g"], lv["pos"], lv["vel"], lv["ldj"], ptr, kBT, softening, 10.0)
        loss.backward()
        res.append((float(loss.detach()), {k: v.grad.double().numpy() for k, v in lv.items()}))
    return b, ldj, res[0], _assert_f32_floor(f"nll kBT {kBT:.3g} softening {softening}", *res)


def _nll_cases():
    from enflow_amd.data.synthetic import default_kBT
    return [(default_kBT(), 0.1), (1.0, 0.0)]


@pytest.mark.parametrize("which", [0, 1], ids=["kBT300K-soft0.1", "kBT1-soft0-coincident"])
def test_alchemical_nll_backward_alone(which):
    from enflow_amd.flow import Alchemical_NLL
    kBT, softening = _nll_cases()[which]
    b, ldj, ref, floor = _nll_alone(kBT, softening)
    data, leaves = _gpu_batch(b, floor_h=True)
    leaves["ldj"] = torch.tensor(ldj, dtype=torch.float32, device="cuda", requires_grad=True)
    loss = 0.37 * Alchemical_NLL(kBT=kBT, softening=softening)(data, leaves["ldj"])
    loss.backward()
    torch.cuda.synchronize()
    got = {k: v.grad.double().cpu().numpy() for k, v in leaves.items()}
    _compare(f"nll alone kBT {kBT:.3g} softening {softening}", float(loss.detach()), got, ref, floor)
