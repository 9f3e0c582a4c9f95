"""Longest-first launch order of the whole-tile flow instances
(enflow_set_longest_first): block b of the flow launch runs the molecule with
the b-th largest unique-pair count at the call's input positions (key and
stable sort on the device).  Only the block-to-molecule map changes,
so every output is bitwise the batch-order launch's; the key is the
reference's unique (row, col) pair count of Data.edges (enflow/data/base.py:
122-144) at those positions."""
import numpy as np
import pytest
import torch

from oracle import enflow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = {"small": [1, 2, 22, 5, 31], "mixed64": [32, 33, 64]}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(params=["4-wave", "8-wave"])
def whole_tile(request):
    """The two whole-tile instances of the <= 32-atom flow kernel, the
    feature-split ones off (larger molecules run the 4-wave 64-atom image)."""
    from enflow_amd import _lib
    prev = (_lib.set_latency_threshold(1 << 30 if request.param == "8-wave" else 0),
            _lib.set_split_threshold(0), _lib.set_fs_threshold(0))
    yield request.param
    _lib.set_latency_threshold(-1 if prev[0] is None else prev[0])
    _lib.set_split_threshold(-1 if prev[1] is None else prev[1])
    _lib.set_fs_threshold(-1 if prev[2] is None else prev[2])


class _mode:
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


def _batch(sizes, seed):
    from enflow_amd.data.synthetic import make_molecules
    return _f32(make_molecules(len(sizes), list(sizes), nf=5, seed=seed))


def _model(hid, n_layers, seed, prec="f16x3"):
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    torch.manual_seed(seed)
    m = LFIntegrator([EGCL(5, 5, hid) for _ in range(n_layers)], ArgMax(5, hid), dt=default_dt()).to(DEV)
    m.gemm_precision = prec
    return m


def _forward(model, b, eps, mode):
    """One raw forward launch (no host retry) under `mode`: outputs, per-molecule
    and batch log|detJ|, the error word, and the kernels launched."""
    from enflow_amd import _lib
    from enflow_amd.data import Data
    s = model._state(Data.from_arrays(b, device=DEV))
    M = s["mol_ptr"].numel() - 1
    ldj_mol, ldj = torch.zeros(max(M, 1), device=DEV), torch.zeros(1, device=DEV)
    st = torch.zeros(2, dtype=torch.int32, device=DEV)
    with _mode(mode), _lib.KernelTimer() as t, torch.no_grad():
        model.forward_buffers(s["h"], s["g"], s["pos"], s["vel"], s["box"], s["r_cut"], s["mol_ptr"], s["max_n"],
                              eps, ldj_mol, ldj, st[:1], src=s["src"], noise_key=(0x5eed, 7), ticket=st[1:])
    torch.cuda.synchronize()
    out = {k: s[k].clone() for k in ("h", "g", "pos", "vel")}
    out.update(ldj_mol=ldj_mol, ldj=ldj, err=st[:1].clone(), ticket=st[1:].clone())
    return out, set(t.stats)


def _reverse(model, b, state, mode):
    from enflow_amd import _lib
    from enflow_amd.data import Data
    s = model._state(Data.from_arrays(b, device=DEV))
    src = tuple(state[k] for k in ("h", "g", "pos", "vel"))
    idx = torch.zeros(max(src[0].shape[0], 1), dtype=torch.int32, device=DEV)
    rv = torch.zeros(2, dtype=torch.int32, device=DEV)
    with _mode(mode), _lib.KernelTimer() as t, torch.no_grad():
        model.reverse_buffers(s["h"], s["g"], s["pos"], s["vel"], s["box"], s["r_cut"], s["mol_ptr"], s["max_n"],
                              idx, rv[1:], rv[:1], src=src)
    torch.cuda.synchronize()
    out = {k: s[k].clone() for k in ("h", "g", "pos", "vel")}
    out.update(argmax_idx=idx, max_idx=rv[1:].clone(), err=rv[:1].clone())
    return out, set(t.stats)


def _assert_same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs between longest-first and batch order"


def _oracle_keys(b):
    keys = []
    for m in range(len(b["mol_ptr"]) - 1):
        a0, a1 = int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1])
        e = O.molecule_edges(b["pos"][a0:a1], b["box"][a0], float(b["r_cut"][m]))
        r, _, _ = O.pair_multiplicity(e[:, 0], e[:, 1], max(a1 - a0, 1))
        keys.append(len(r))
    return np.array(keys, dtype=np.int64)


def _diag(b, **kw):
    from enflow_amd import _lib
    sizes = np.diff(b["mol_ptr"])
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV).contiguous()
    keys, order, applied = _lib.longest_first_order(t(b["mol_ptr"], torch.int32), t(b["r_cut"], torch.float32),
                                                    t(b["box"], torch.float32), t(b["pos"], torch.float32),
                                                    int(sizes.max()) if len(sizes) else 0, **kw)
    torch.cuda.synchronize()
    return keys.cpu().numpy().astype(np.int64), order.cpu().numpy().astype(np.int64), applied


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("draws", ["kernel", "caller"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_longest_first_is_bitwise_batch_order(name, draws, prec, whole_tile):
    """Forward and reverse under mode 2 (always) against mode 0: h, g, pos, vel,
    per-molecule and batch log|detJ|, the ArgMax indices and the error words
    bitwise equal, on the 4-wave and 8-wave instances, f16x3 and f32 GEMMs, with
    in-kernel draws (same key) and the caller's noise."""
    b = _batch(BATCHES[name], 70)
    model = _model(128, 2, 71, prec)
    eps = (torch.randn((b["h"].shape[0], 5), device=DEV, generator=torch.Generator(DEV).manual_seed(72))
           if draws == "caller" else None)
    f2, k2 = _forward(model, b, eps, 2)
    f0, k0 = _forward(model, b, eps, 0)
    assert "order_key_kernel" in k2 and "order_rank_kernel" in k2 and "order_key_kernel" not in k0, (k2, k0)
    assert not any(k.startswith("lf_fs_kernel") for k in k2 | k0), (k2, k0)
    _assert_same(f2, f0, f"forward [{whole_tile}] {name} {draws} {prec}")
    assert int(f0["ticket"]) == 0 and bool(torch.isfinite(f0["ldj"]).all())
    r2, q2 = _reverse(model, b, f0, 2)
    r0, q0 = _reverse(model, b, f0, 0)
    assert "order_key_kernel" in q2 and "order_key_kernel" not in q0, (q2, q0)
    _assert_same(r2, r0, f"reverse [{whole_tile}] {name} {draws} {prec}")
    print(f"[{whole_tile}] {name} {draws} {prec}: forward + reverse bitwise equal, err words "
          f"{int(f2['err'])} / {int(r2['err'])}")


def test_batches_with_nothing_to_order(whole_tile):
    """No molecule (the flow entry launches nothing for it: the diagnostic entry
    returns empty arrays), one molecule, all keys equal (one molecule repeated),
    molecules without a pair and r_cut below every distance: the order is the
    stable one (batch order where the keys are equal) and the outputs are the
    batch-order launch's."""
    from enflow_amd.data.synthetic import make_molecules
    model = _model(64, 2, 73)
    one = _batch([22], 74)
    rep = _f32(make_molecules(6, 22, nf=5, seed=75))
    n = 22
    for k in ("h", "g", "pos", "vel", "box"):      # six copies of the first molecule
        rep[k] = np.tile(rep[k][:n], (6, 1))
    rep["r_cut"] = np.repeat(rep["r_cut"][:1], 6)
    lonely = _batch([22, 5, 1, 9], 76)
    lonely["r_cut"] = np.full_like(lonely["r_cut"], 1e-3)
    empty = {k: v[:0] for k, v in one.items() if k not in ("mol_ptr", "r_cut")}
    empty.update(mol_ptr=np.zeros(1, dtype=one["mol_ptr"].dtype), r_cut=one["r_cut"][:0])
    keys, order, applied = _diag(empty)
    assert keys.size == 0 and order.size == 0
    # r_cut below every distance: an atom is then hit only by itself, which the
    # reference still lists where id_mapping relabels the hit (base.py:137-139),
    # so only the one-atom molecules are certain to have no pair at all
    single = _batch([1, 1, 1, 1], 84)
    single["r_cut"] = np.full_like(single["r_cut"], 1e-3)
    for name, b in (("one", one), ("equal keys", rep), ("no pairs", single), ("tiny r_cut", lonely)):
        M = len(b["mol_ptr"]) - 1
        with _mode(2):
            keys, order, applied = _diag(b)
        assert applied and np.array_equal(keys, _oracle_keys(b)), (name, keys, _oracle_keys(b))
        assert np.array_equal(order, np.argsort(-keys, kind="stable")), (name, keys, order)
        if name == "tiny r_cut":
            assert keys[2] == 0 and keys.max() <= 22, keys      # the one-atom molecule; no real neighbour anywhere
        else:
            assert np.array_equal(order, np.arange(M)), (name, keys, order)
            assert len(set(keys.tolist())) == 1, (name, keys)
        if name == "no pairs":
            assert not keys.any()
        f2, k2 = _forward(model, b, None, 2)
        f0, _ = _forward(model, b, None, 0)
        assert "order_key_kernel" in k2
        _assert_same(f2, f0, name)
        r2, _ = _reverse(model, b, f0, 2)
        r0, _ = _reverse(model, b, f0, 0)
        _assert_same(r2, r0, name + " reverse")


def test_key_is_the_oracle_unique_pair_count():
    """40 x 22 atoms plus molecules of 1, 2, 31 and 32 atoms: the device key of
    every molecule equals the unique (row, col) pairs of the oracle's
    molecule_edges + pair_multiplicity at the input positions, exactly; the
    64-atom image's key kernel likewise on a batch with larger molecules."""
    b = _batch([22] * 40 + [1, 2, 31, 32], 78)
    want = _oracle_keys(b)
    keys, order, _ = _diag(b)
    print("keys", keys.tolist())
    assert np.array_equal(keys, want), (keys - want).tolist()
    assert want[:40].min() < want[:40].max()            # the 22-atom molecules do differ
    b64 = _batch([33, 64, 22, 1, 50], 79)
    keys64, _, _ = _diag(b64)
    assert np.array_equal(keys64, _oracle_keys(b64)), (keys64, _oracle_keys(b64))


@pytest.mark.parametrize("sizes", [[22] * 40 + [1, 2, 31, 32], [5, 6, 7] * 100, [2, 3, 4, 3] * 275,
                                   [33, 64, 22, 1, 50]], ids=["44mols", "300mols", "1100mols", "64image"])
def test_order_is_a_stable_descending_permutation(sizes):
    """The order is a permutation of the molecules, sorted by key descending,
    ties in molecule order (300 molecules: more than one workgroup of the rank
    kernel; 1100: more than one of its comparison chunks), and the same over two calls."""
    b = _batch(sizes, 80)
    keys, order, _ = _diag(b)
    keys2, order2, _ = _diag(b)
    M = len(sizes)
    assert np.array_equal(np.sort(order), np.arange(M))
    assert np.array_equal(order, np.argsort(-keys, kind="stable"))
    assert np.array_equal(keys, keys2) and np.array_equal(order, order2)


def test_fp32_rerun_of_a_flagged_molecule_ignores_the_order(whole_tile):
    """One molecule whose GEMM operands are all ~1e-4 (tests/test_gpu_small.py's
    construction) in a batch of 16: the f16x3 launch names it
    (ENFLOW_ERR_SMALL), the host re-runs it alone with fp32 GEMMs through a
    molecule list -- which ignores the order.  Module outputs under mode 2 equal
    mode 0's bitwise."""
    from enflow_amd import _lib
    from enflow_amd.nn import EGCL, Floor
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data import Data
    from enflow_amd.data.synthetic import make_molecules, default_dt
    k = 5
    small = _f32(make_molecules(16, 22, nf=5, seed=61))
    small["h"] = np.floor(np.random.default_rng(62).uniform(0, 3, size=small["h"].shape))
    a0, a1 = int(small["mol_ptr"][k]), int(small["mol_ptr"][k + 1])
    for key, f in (("h", 1e-4), ("g", 1e-4), ("pos", 1e-3), ("vel", 1e-3), ("box", 1e-3)):
        small[key][a0:a1] = small[key][a0:a1] * f
    small["r_cut"][k] = small["r_cut"][k] * 1e-3
    small = _f32(small)
    torch.manual_seed(63)
    model = LFIntegrator([EGCL(5, 5, 128) for _ in range(3)], Floor(dequant_scale=1e-4), dt=default_dt()).to(DEV)
    u = torch.rand(small["h"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(64))
    res = {}
    for mode in (2, 0):
        n0, m0 = _lib.FP32_RERUNS[0], _lib.FP32_MOL_RERUNS[0]
        with _mode(mode), torch.no_grad():
            o, ldj = model(Data.from_arrays(small, device=DEV), noise=u)
        torch.cuda.synchronize()
        assert (_lib.FP32_RERUNS[0] - n0, _lib.FP32_MOL_RERUNS[0] - m0) == (1, 1), f"mode {mode}"
        res[mode] = dict(h=o.h, g=o.g, pos=o.pos, vel=o.vel, ldj=ldj)
    _assert_same(res[2], res[0], f"[{whole_tile}] flagged-molecule re-run")


def test_auto_mode_leaves_a_small_batch_in_batch_order():
    """Auto (mode 1) orders only launches with more molecules than resident
    workgroup slots (two per CU): a 40-molecule batch reports "not applied" and
    launches no key kernel; mode 2 reports applied, mode 0 never."""
    from enflow_amd import _lib
    b = _batch([22] * 40, 81)
    model = _model(128, 1, 82)
    prev = (_lib.set_latency_threshold(0), _lib.set_split_threshold(0), _lib.set_fs_threshold(0))
    try:
        with _mode(1):
            _, _, applied = _diag(b)
            assert not applied
        _, launched = _forward(model, b, None, 1)
        assert "order_key_kernel" not in launched, launched
        with _mode(2):
            assert _diag(b)[2] and _diag(b, reverse=True)[2] and _diag(b, training=True)[2]
        with _mode(0):
            assert not _diag(b)[2]
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        big = _batch([3] * (2 * cus + 1), 83)
        with _mode(1):
            assert _diag(big)[2] and _diag(big, reverse=True)[2] and not _diag(big, training=True)[2]
            assert not _diag(_batch([3] * (2 * cus), 83))[2]
    finally:
        _lib.set_latency_threshold(-1 if prev[0] is None else prev[0])
        _lib.set_split_threshold(-1 if prev[1] is None else prev[1])
        _lib.set_fs_threshold(-1 if prev[2] is None else prev[2])
