"""EGCL.forward_edges: EGCL on a caller-supplied edge list with the HIP backward
(enflow_egcl_forward_list_tape_f32, lf_layer_bwd_kernel<.., LIST>, el_colsum_kernel,
enflow_egcl_backward_list_f32), from the kernels up to the module.

Reference: the float64 torch restatement of egcl.py:57-92 in tests/_edge_list_grad.py
(pinned to the oracles by tests/test_edge_list_grad_host.py), fed what the device is
fed (fp32 weights, features and coord_diff).  Bars: GRAD_TOL = 5e-5 normwise per
gradient tensor, 1e-5 per output tensor.  Every case first asserts on the CPU that
the same restatement in float32 is within half the bar of its float64 run (the
floor), so the bar tests the kernels and not the inputs' conditioning.  Worst
errors and floors are printed (DESIGN.md section 3h records them)."""
import numpy as np
import pytest
import torch
from torch import nn

from _fixtures import load, data_from_fixture, egcl_from_fixture, normwise, worst_of, assert_all_within
from _edge_list_grad import List, case_inputs, rand_weights, restate, scatter_to_pos, weighted
from test_gpu_train import GRAD_TOL
from enflow_amd import _lib
from enflow_amd.nn import EGCL
from enflow_amd.flow._train import egcl_list_backward

pytestmark = pytest.mark.gpu
OUT_TOL = 1e-5
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def reference(net, h, row, col, cd, w, what):
    """(outs, grads) of the float64 restatement, after the float32 floor."""
    ref = restate(net, h, row, col, cd, w)
    r32 = restate(net, h, row, col, cd, w, dtype=torch.float32)
    floor = {k: normwise(r32[1][k], v) for k, v in ref[1].items()}
    ofloor = {k: normwise(r32[0][k], v) for k, v in ref[0].items()}
    print(f"{what}: float32-restatement floor {worst_of(floor):.2e} (outputs {worst_of(ofloor):.2e})")
    assert_all_within(floor, GRAD_TOL / 2, f"{what}: float32 restatement vs float64")
    assert_all_within(ofloor, OUT_TOL / 2, f"{what}: float32 restatement outputs vs float64")
    return ref


def run(net, h, row, col, cd, w, itype=torch.int64, ftype=torch.float32):
    """forward_edges + backward on the device: (outs, grads, the coord_diff leaf)."""
    for p in net.parameters():
        p.grad = None
    ht = torch.tensor(h, device=DEV).requires_grad_(True)
    cdt = torch.tensor(cd, device=DEV).to(ftype).reshape(-1, 3).requires_grad_(True)
    lst = List(torch.tensor(row, device=DEV).to(itype), torch.tensor(col, device=DEV).to(itype), cdt)
    outs = net.forward_edges(ht, lst)
    wt = [None if x is None else torch.tensor(x, device=DEV) for x in w]
    weighted(outs, wt).backward()
    own = net.act_param_ids()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().cpu().numpy()   # noqa: E731
    grads = {"h": z(ht), "coord_diff": z(cdt)}
    grads.update({k: z(p) for k, p in net.named_parameters() if id(p) not in own})
    return {k: o.detach().double().cpu().numpy() for k, o in zip("QFG", outs)}, grads, cdt


def compare(what, got, ref, tol=GRAD_TOL):
    oerr = {k: normwise(got[0][k], v) for k, v in ref[0].items()}
    gerr = {k: normwise(got[1][k], v) for k, v in ref[1].items()}
    print(f"{what}: worst gradient {worst_of(gerr):.2e}, worst output {worst_of(oerr):.2e}")
    assert_all_within(oerr, OUT_TOL, f"{what} outputs")
    assert_all_within(gerr, tol, f"{what} gradients")
    return worst_of(gerr)


def module(seed, nf_in=5, nf_out=5, hid=32, **kw):
    """Module-init weights from a seed."""
    torch.manual_seed(seed)
    net = EGCL(nf_in, nf_out, hid, **kw)
    for q in net.act_fn.parameters():
        q.requires_grad_(False)              # a PReLU slope: frozen, as everywhere (check_trainable)
    return net.to(DEV)


# ---------------------------------------------------------------------------
# 1. the goldens through Edges.reference(): restatement, handle path
# ---------------------------------------------------------------------------
_golden = {}


def golden(name):
    if name not in _golden:
        inp, _ = load(name)
        nf, hid = inp["h"].shape[1], int(inp["p0.edge_nn.2.weight"].shape[0])
        net = egcl_from_fixture(inp, 0, nf, hid).to(DEV)
        d = data_from_fixture(inp, DEV)
        _golden[name] = (net, d, d.edges.reference())
    return _golden[name]


@pytest.mark.parametrize("name", ["egcl_h32", "egcl_h128_all"])
def test_goldens_vs_restatement_and_handle_path(name):
    net, d, ref_list = golden(name)
    n, nf = d.h.shape
    row, col = ref_list.row.cpu().numpy(), ref_list.col.cpu().numpy()
    cd, h = ref_list.coord_diff.float().cpu().numpy(), d.h.cpu().numpy()
    w = rand_weights(n, nf)
    ref = reference(net, h, row, col, cd, w, name)
    got = run(net, h, row, col, cd, w)
    compare(f"{name} list vs restatement", got, ref)
    # the Data.edges handle path's backward on the same batch
    for p in net.parameters():
        p.grad = None
    d2 = data_from_fixture(load(name)[0], DEV)
    ht, pt = d2.h.requires_grad_(True), d2.pos.requires_grad_(True)
    outs = net(ht, d2.edges)
    weighted(outs, [torch.tensor(x, device=DEV) for x in w]).backward()
    hgrads = {"h": ht.grad.double().cpu().numpy()}
    hgrads.update({k: p.grad.double().cpu().numpy() for k, p in net.named_parameters()})
    herr = {k: normwise(got[1][k], v) for k, v in hgrads.items()}
    herr["pos"] = normwise(scatter_to_pos(n, row, col, got[1]["coord_diff"]), pt.grad.double().cpu().numpy())
    print(f"{name} list vs handle path: worst {worst_of(herr):.2e}")
    assert_all_within(herr, GRAD_TOL, f"{name} list vs handle path")


# ---------------------------------------------------------------------------
# 2. synthetic graphs, random adjoints on Q, F and G
# ---------------------------------------------------------------------------
# (graph, module keywords)
SYNTHETIC = [
    ("n1_no_edges", dict()),
    ("n33_two_blocks_empty_rows", dict()),
    ("row_of_200_edges", dict()),
    ("row_of_200_edges", dict(hid=128, attention=True, norm_diff=True, tanh=True)),
    ("two_passes_1280_edges", dict()),
    ("two_passes_1280_edges", dict(hid=64, attention=True)),
    ("columns_in_other_blocks", dict()),
    ("repeats_and_self_loops", dict()),
    ("column_only_and_never_column", dict()),
    ("hub", dict()),
    ("hub", dict(hid=128)),
    ("random_20", dict(nf_out=3)),
    ("random_20", dict(hid=48)),
    ("random_20", dict(nf_in=16, nf_out=16, hid=128)),
    ("random_20", dict(act_fn=nn.GELU())),
    ("random_20", dict(act_fn=nn.PReLU(init=0.2))),
]


def _sid(s):
    kw = {k: (type(v).__name__ if isinstance(v, nn.Module) else v) for k, v in s[1].items()}
    return s[0] + "".join(f"-{k}={v}" for k, v in kw.items())


@pytest.mark.parametrize("kind,kw", SYNTHETIC, ids=[_sid(s) for s in SYNTHETIC])
def test_synthetic_graphs_vs_restatement(kind, kw):
    net = module(7, **kw)
    n, row, col, cd, h = case_inputs(kind, net.input_nf)
    w = rand_weights(n, net.output_nf)
    ref = reference(net, h, row, col, cd, w, _sid((kind, kw)))
    got = run(net, h, row, col, cd, w, itype=torch.int32)
    assert got[1]["h"].shape == (n, net.input_nf) and got[1]["coord_diff"].shape == (row.size, 3)
    compare(_sid((kind, kw)), got, ref)


@pytest.mark.parametrize("kind", ["n1_no_edges", "n40_no_edges"])
def test_no_edges_edge_gradients_are_exactly_zero(kind):
    net = module(7)
    n, row, col, cd, h = case_inputs(kind, 5)
    w = rand_weights(n, 5)
    ref = reference(net, h, row, col, cd, w, kind)
    got = run(net, h, row, col, cd, w)
    for k, v in got[1].items():
        if k.startswith(("edge_nn.", "coord_nn.")):
            assert not v.any(), k
    compare(kind, got, ref)


def test_shuffled_int64_fp64_list_returns_d_coord_diff_in_the_callers_order_and_dtype():
    net = module(7)
    n, row, col, cd, h = case_inputs("random_20", 5)      # case_inputs shuffles the list
    assert np.any(np.diff(row) < 0)
    w = rand_weights(n, 5)
    ref = reference(net, h, row, col, cd, w, "shuffled")
    got = run(net, h, row, col, cd, w, itype=torch.int64, ftype=torch.float64)
    assert got[2].grad.dtype == torch.float64 and got[2].grad.shape == (row.size, 3)
    compare("shuffled int64 / fp64", got, ref)


@pytest.mark.parametrize("which", ["only_G", "only_Q", "only_F"])
def test_partial_upstreams(which):
    net = module(7)
    n, row, col, cd, h = case_inputs("random_20", 5)
    wq, wf, wg = rand_weights(n, 5)
    w = {"only_G": (None, None, wg), "only_Q": (wq, None, None), "only_F": (None, wf, None)}[which]
    ref = reference(net, h, row, col, cd, w, which)
    got = run(net, h, row, col, cd, w)
    compare(which, got, ref)
    if which == "only_Q":      # nothing reaches the edges
        for k, v in got[1].items():
            if k.startswith(("edge_nn.", "coord_nn.", "node_nn.")) or k == "coord_diff":
                assert not v.any(), k


def test_none_adjoints_give_zero_gradients():
    net = module(7)
    n, row, col, cd, h = case_inputs("random_20", 5)
    t = lambda a: torch.tensor(a, device=DEV)   # noqa: E731
    dh, dcd, grad = egcl_list_backward(net, t(h), t(row), t(col), t(cd), None, None, None)
    assert dh.shape == (n, 5) and dcd.shape == (row.size, 3)
    assert not dh.any() and not dcd.any() and not grad.any()


# ---------------------------------------------------------------------------
# 3. the f16x3 instance, determinism, forward identities, the index guard
# ---------------------------------------------------------------------------
def test_f16x3_instance_on_egcl_h128():
    inp, _ = load("egcl_h128")
    net = egcl_from_fixture(inp, 0, inp["h"].shape[1], 128).to(DEV)
    d = data_from_fixture(inp, DEV)
    lst = d.edges.reference()
    n, nf = d.h.shape
    row, col = lst.row.cpu().numpy(), lst.col.cpu().numpy()
    cd, h = lst.coord_diff.float().cpu().numpy(), d.h.cpu().numpy()
    w = rand_weights(n, nf)
    ref = reference(net, h, row, col, cd, w, "egcl_h128")
    adj = [torch.tensor(x, device=DEV) for x in w]
    errs = {}
    for prec, tag in ((_lib.PREC_F32, "f32"), (_lib.PREC_F16X3, "f16x3")):
        dh, dcd, grad, e = egcl_list_backward(net, d.h, lst.row, lst.col, lst.coord_diff, *adj, prec=prec,
                                              return_err=True)
        assert e == 0, f"{tag}: error word {e}"
        from enflow_amd.flow._train import layer_grads
        got = {"h": dh.double().cpu().numpy(), "coord_diff": dcd.double().cpu().numpy()}
        got.update({k: g.double().cpu().numpy() for (k, _), g in zip(net.named_parameters(), layer_grads(net, grad))})
        errs[tag] = {k: normwise(got[k], v) for k, v in ref[1].items()}
        print(f"egcl_h128 {tag} list backward: worst {worst_of(errs[tag]):.2e}")
        assert_all_within(errs[tag], GRAD_TOL, f"egcl_h128 {tag}")
    # tests/test_gpu_train.py's rule for the split precision against the fp32 path
    assert worst_of(errs["f16x3"]) <= 1.25 * worst_of(errs["f32"]) + 1e-6, errs


def test_two_backward_calls_are_bitwise_equal():
    net = module(7, hid=64, attention=True)
    n, row, col, cd, h = case_inputs("hub", 5)
    w = rand_weights(n, 5)
    a = run(net, h, row, col, cd, w)[1]
    b = run(net, h, row, col, cd, w)[1]
    for k in a:
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k


def test_forward_identities_and_index_guard():
    net = module(7)
    n, row, col, cd, h = case_inputs("two_passes_1280_edges", 5)
    t = lambda a: torch.tensor(a, device=DEV)   # noqa: E731
    lst = List(t(row), t(col), t(cd))
    ht = t(h)
    with torch.no_grad():
        a = net.forward_edges(ht, lst)
        b = net(ht, lst)
    c = net.forward_edges(ht.clone().requires_grad_(True), lst)     # the autograd Function's forward
    *taped, tape, _ = net._infer_list(ht, lst.row, lst.col, lst.coord_diff, tape=True)
    for x, y, z, u in zip(a, b, c, taped):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert torch.equal(x.view(torch.int32), z.detach().view(torch.int32))
        assert torch.equal(x.view(torch.int32), u.view(torch.int32))
    # the tape holds the h rows and Q
    hx = tape[:n * (5 + 32)].reshape(n, 37)
    assert torch.equal(hx[:, :5], ht)
    for bad in (n, -1):
        colb = t(col).clone()
        colb[7] = bad
        with pytest.raises(IndexError):
            net.forward_edges(ht.clone().requires_grad_(True), List(lst.row, colb, lst.coord_diff))
    rowb = t(row).clone()
    rowb[3] = n
    with pytest.raises(IndexError):
        net.forward_edges(ht.clone().requires_grad_(True), List(rowb, lst.col, lst.coord_diff))
    with pytest.raises(NotImplementedError, match="forward_edges"):   # forward keeps refusing, and points here
        net(ht.clone().requires_grad_(True), lst)
