"""hidden_nf 129..256 on the host: the reference-made golden at width 256 pins
the oracle there, zero-padding 160 -> 256 is exact, wide_hidden's values and
every refusal's message.  No GPU."""
import numpy as np
import pytest
import torch
from torch import nn

from _fixtures import state
from _wide import golden_model, oracle_params
from oracle import enflow_oracle as O


def test_oracle_reproduces_the_width_256_golden():
    model, inp, gold = golden_model("cpu")
    layers = [oracle_params(n) for n in model.networks]
    dq = oracle_params(model.dequantize)
    ref, ldj = O.lf_forward(layers, dq, state(inp), inp["eps"].astype(np.float64), float(inp["dt"]))
    for k in ("h", "g", "pos", "vel"):
        np.testing.assert_allclose(ref[k], gold[k], rtol=1e-12, atol=1e-12, err_msg=k)
    assert abs(ldj - float(gold["ldj"])) <= 1e-12 * abs(float(gold["ldj"]))
    nll = O.alchemical_nll(ref, ldj, float(inp["kBT"]), float(inp["softening"]))
    assert abs(nll - float(gold["nll"])) <= 1e-12 * abs(float(gold["nll"]))
    st = {k: gold[k] for k in ("h", "g", "pos", "vel")}
    st.update(box=inp["box"].astype(np.float64), r_cut=inp["r_cut"].astype(np.float64), mol_ptr=inp["mol_ptr"])
    back = O.lf_reverse(layers, st, float(inp["dt"]))
    assert np.array_equal(back["h"], gold["rev_h"])
    for k in ("g", "pos", "vel"):
        np.testing.assert_allclose(back[k], gold["rev_" + k], rtol=1e-12, atol=1e-12, err_msg=k)


def test_seeded_weights_and_state_dict_keys_at_256():
    """golden_model checks every parameter against the reference's fingerprint."""
    model, inp, gold = golden_model("cpu")
    keys = {k[3:-3] for k in gold if k.startswith("p0.") and k.endswith(".fp")}
    assert keys == set(model.networks[0].state_dict().keys())
    assert {k[3:-3] for k in gold if k.startswith("dq.")} == set(model.dequantize.state_dict().keys())


@pytest.mark.parametrize("act", [nn.SiLU(), nn.Sigmoid(), nn.Softplus()])
def test_padding_160_to_256_is_exact(act):
    """The zero-padded 256-wide parameters give the 160-wide network's outputs
    (act(0) != 0 for Sigmoid / Softplus: a padded unit still reaches no output)."""
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.nn._pad import wide_hidden
    from enflow_amd.nn._act import act_code
    H, nf = 160, 5
    Hp = wide_hidden(H)
    assert Hp == 256
    torch.manual_seed(160)
    net = EGCL(nf, nf, H, act_fn=act, attention=True).double()
    assert net.kernel_hidden == 256 and net.wide
    flat = net.kernel_raw("cpu").double().numpy()
    att = net._att_raw("cpu").double().numpy()
    shapes = {"edge_nn.0.weight": (Hp, 2 * nf + 1), "edge_nn.0.bias": (Hp,), "edge_nn.2.weight": (Hp, Hp),
              "edge_nn.2.bias": (Hp,), "node_nn.0.weight": (Hp, Hp + nf), "node_nn.0.bias": (Hp,),
              "node_nn.2.weight": (nf, Hp), "node_nn.2.bias": (nf,), "coord_nn.0.weight": (Hp, Hp),
              "coord_nn.0.bias": (Hp,), "coord_nn.2.weight": (1, Hp), "vel_scaling_nn.0.weight": (Hp, nf),
              "vel_scaling_nn.0.bias": (Hp,), "vel_scaling_nn.2.weight": (1, Hp), "vel_scaling_nn.2.bias": (1,)}
    padded, off = {}, 0
    for k in O.EGCL_PARAM_NAMES:      # the raw vector's order
        n = int(np.prod(shapes[k]))
        padded[k] = flat[off:off + n].reshape(shapes[k]).astype(np.float64)
        off += n
    assert off == flat.size
    padded["att_nn.0.weight"], padded["att_nn.0.bias"] = att[:Hp].reshape(1, Hp), att[Hp:]
    real = oracle_params(net)
    padded["flags"] = real["flags"]
    if "act" in real:
        padded["act"] = real["act"]
    # float32 parameters on both sides (kernel_raw is fp32)
    real = {k: (v.astype(np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in real.items()}
    rng = np.random.default_rng(1)
    n, E = 30, 200
    h = rng.normal(size=(n, nf))
    row, col = np.sort(rng.integers(0, n, E)), rng.integers(0, n, E)
    cd = rng.normal(size=(E, 3))
    a = O.egcl_forward(real, h, row, col, cd)
    b = O.egcl_forward(padded, h, row, col, cd)
    for x, y in zip(a, b):
        np.testing.assert_allclose(y, x, rtol=1e-12, atol=1e-13)
    # ArgMax, padded by the flow to its layers' width
    am = ArgMax(nf, H, act_fn=act).double()
    rawa = am.kernel_raw("cpu", 256).double().numpy()
    pa = {"network.0.weight": rawa[:Hp * nf].reshape(Hp, nf), "network.0.bias": rawa[Hp * nf:Hp * nf + Hp],
          "network.2.weight": rawa[Hp * nf + Hp:Hp * nf + Hp + 2 * nf * Hp].reshape(2 * nf, Hp),
          "network.2.bias": rawa[Hp * nf + Hp + 2 * nf * Hp:Hp * nf + Hp + 2 * nf * Hp + 2 * nf]}
    ra = {k: (v.astype(np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v)
          for k, v in oracle_params(am).items()}
    if "act" in ra:
        pa["act"] = ra["act"]
    assert act_code(act) == am.act()
    hq, eps = np.eye(nf)[rng.integers(0, nf, n)], rng.normal(size=(n, nf))
    z0, l0 = O.argmax_forward(ra, hq, eps)
    z1, l1 = O.argmax_forward(pa, hq, eps)
    np.testing.assert_allclose(z1, z0, rtol=1e-12, atol=1e-13)
    assert abs(l1 - l0) <= 1e-12 * abs(l0)


def test_wide_hidden_values_and_kernel_hidden_unchanged():
    from enflow_amd.nn._pad import kernel_hidden, wide_hidden, run_hidden
    assert kernel_hidden(129) is None and kernel_hidden(256) is None and kernel_hidden(128) == 128
    assert [wide_hidden(x) for x in (1, 128, 129, 160, 255, 256, 257)] == [None, None, 256, 256, 256, 256, None]
    assert run_hidden(100) == 128 and run_hidden(200) == 256 and run_hidden(300) is None


def test_library_answers_for_256():
    from enflow_amd import _lib
    for nf, L in ((5, _lib.lib()), (12, _lib.lib(16))):
        assert L.enflow_supports_wide_hidden(256) == 1 and L.enflow_supports_wide_hidden(128) == 0
        assert L.enflow_supports_hidden(256) == 0
        assert L.enflow_egcl_packed_size(256, nf) == L.enflow_egcl_wide_packed_size(256, nf) > 2 * 256 * 256
        assert L.enflow_egcl_packed_size(512, nf) == -1 and L.enflow_argmax_packed_size(256, nf) > 0
        # the fused entries refuse the width (-5) before touching any pointer
        assert L.enflow_egcl_forward_f32(1, 4, 4, nf, 256, *([None] * 6), 1.0, *([None] * 5)) == -5


def test_refusals_and_messages():
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data import Data
    assert EGCL(5, 5, 256).hip_supported() and EGCL(5, 5, 129).hip_supported() and EGCL(12, 12, 200).hip_supported()
    assert not EGCL(5, 5, 257).hip_supported()
    with pytest.raises(NotImplementedError, match="hidden_nf <= 256"):
        EGCL(5, 5, 257)._check_supported()
    net = EGCL(5, 5, 256)
    h = torch.zeros(4, 5)
    d = Data(h=h, g=h.clone(), pos=torch.zeros(4, 3), vel=torch.zeros(4, 3), N=torch.tensor([4]),
             r_cut=torch.tensor([1.0]), box=torch.ones(4, 3), device="cpu")
    msg = r"inference only at hidden_nf > 128: call under torch\.no_grad\(\)"
    with pytest.raises(NotImplementedError, match=msg):
        net(h, d.edges)
    with pytest.raises(NotImplementedError, match=msg):
        ArgMax(5, 256)(h)

    class List:
        row = col = torch.zeros(1, dtype=torch.long)
        coord_diff = torch.zeros(1, 3)
    with pytest.raises(NotImplementedError, match="caller-supplied edge list.*up to hidden_nf 128"):
        with torch.no_grad():
            net(h, List())
    with pytest.raises(NotImplementedError, match=msg):
        net.forward_edges(h, List())
    model = LFIntegrator([EGCL(5, 5, 200), EGCL(5, 5, 200)], ArgMax(5, 200), dt=0.01)
    for call in (model, model.forward_grad, model.reverse_grad):
        with pytest.raises(NotImplementedError, match=msg):
            call(d)
    with pytest.raises(NotImplementedError, match="hidden_nf <= 256"):
        LFIntegrator([EGCL(5, 5, 300)], None, dt=0.01)._geometry()


def test_reference_round_trip_of_g_on_the_golden_batch():
    """Why the GPU round trip (test_gpu_wide_hidden.py::test_golden_batch) asserts vel and pos and
    only prints g: the batch's input positions are not wrapped into the box, so the reverse's
    last layer sees other periodic images than the forward's first did.  In float64, on the
    reference's algorithm, vel comes back to 1e-7 and g is off by ~8.9e-4 of its scale."""
    model, inp, gold = golden_model("cpu")
    layers = [oracle_params(n) for n in model.networks]
    ref, _ = O.lf_forward(layers, oracle_params(model.dequantize), state(inp), inp["eps"].astype(np.float64),
                          float(inp["dt"]))
    back = O.lf_reverse(layers, ref, float(inp["dt"]), dequant_kind="none")
    g_err = float(np.max(np.abs(back["g"] - inp["g"])) / np.max(np.abs(ref["g"])))
    v_err = float(np.linalg.norm(back["vel"] - inp["vel"]) / np.linalg.norm(inp["vel"]))
    assert v_err < 1e-7 and 8e-4 < g_err < 1e-3, (v_err, g_err)


def test_bf16_falls_to_f16x3_with_a_warning_at_wide_widths():
    from enflow_amd import _lib
    from enflow_amd.nn import EGCL
    from enflow_amd.flow import LFIntegrator
    model = LFIntegrator([EGCL(5, 5, 256)], None, dt=0.01)
    assert model._prec() == _lib.PREC_F16X3
    model.gemm_precision = "bf16"
    with pytest.warns(RuntimeWarning, match="bf16.*runs f16x3"):
        assert model._prec() == _lib.PREC_F16X3
    narrow = LFIntegrator([EGCL(5, 5, 128)], None, dt=0.01)
    narrow.gemm_precision = "bf16"
    assert narrow._prec() == _lib.PREC_BF16
