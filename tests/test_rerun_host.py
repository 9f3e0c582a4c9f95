"""CPU-only checks of the host's re-run policy (_rerun in enflow_amd/flow/dynamics.py):
the ladder is driven with CPU int32 words, a fake launch that records
(prec, mol_list) and a scripted sequence of error words; the launches, the
counters' increments and what is raised are compared with the policy of
DESIGN.md section 1, "Error semantics".  No library, no device."""
import pytest
import torch

from enflow_amd import _lib
from enflow_amd.flow.dynamics import _fp32_prec as fp32_prec
from enflow_amd.flow.dynamics import _rerun as rerun
from enflow_amd.flow.dynamics import _retry_fp32 as retry_fp32

F16X3 = _lib.PREC_F16X3 | _lib.EGCL_VARIANTS     # a variant bit, to see that it is kept
F32 = _lib.PREC_F32 | _lib.EGCL_VARIANTS
RANGE, SMALL, HANDOFF, FEW = _lib.ERR_RANGE, _lib.ERR_SMALL, _lib.ERR_HANDOFF, _lib.ERR_FEW_IMAGES
COUNTERS = (_lib.HANDOFF_RERUNS, _lib.FP32_RERUNS, _lib.FP32_MOL_RERUNS)


def drive(words, prec=F16X3, M=8, flagged=(), bit=RANGE, mol_err=True, hooks=False):
    """Read the first scripted word as LFIntegrator.forward / reverse do and
    hand it to the ladder, which reads the others; returns what happened."""
    words = list(words)
    cap = M + 3                                  # the cached words are longer than the batch
    me = None
    if mol_err:
        me = torch.zeros(cap, dtype=torch.int32)
        for m in flagged:
            me[m] = bit
        me[M:] = RANGE                           # past the batch: never a flagged molecule
    log = []                                     # every call the ladder makes, in order
    before = [c[0] for c in COUNTERS]

    def launch(prec, mol_list):
        log.append(("launch", prec, None if mol_list is None else mol_list.tolist()))
        if mol_list is not None:
            assert mol_list.dtype == torch.int32 and mol_list.is_contiguous()
            assert me is None or not me.any()    # zeroed before the re-launch

    def read():
        log.append(("read",))
        return words.pop(0)

    kw = {}
    if hooks:
        kw = dict(zero_handoff=lambda: log.append(("zero_handoff",)),
                  zero_fp32=lambda ml: log.append(("zero_fp32", None if ml is None else ml.tolist())),
                  settle=lambda: log.append(("settle",)))
    raised, out = None, None
    try:
        out = rerun(read(), launch, read, prec, M, me, **kw)
    except (IndexError, FloatingPointError, _lib.HipPathError) as exc:    # what _lib.raise_code raises
        raised = exc
    assert not words, "the ladder read fewer words than scripted"
    return dict(launches=[x[1:] for x in log if x[0] == "launch"], reads=sum(x[0] == "read" for x in log),
                log=log, out=out, raised=raised, mol_err=me,
                counters=tuple(c[0] - b for c, b in zip(COUNTERS, before)))


def test_clean_launch_reads_once():
    r = drive([0], hooks=True)      # the callers skip the ladder on a zero word; it would do nothing
    assert r["launches"] == [] and r["reads"] == 1 and r["raised"] is None
    assert r["out"] == (False, None) and r["counters"] == (0, 0, 0)
    assert r["log"] == [("read",), ("settle",)]


@pytest.mark.parametrize("M,flagged,listed", [
    (8, [5], True),            # one flagged molecule
    (8, [2, 7], True),         # 2 <= 8 // 4
    (8, [0, 3, 4], False),     # 3 > 8 // 4: the whole batch
    (2, [1], True),            # max(1, 2 // 4) = 1
    (2, [0, 1], False),
    (8, [], False),            # the word is set, no molecule is flagged
])
def test_flagged_list_rule(M, flagged, listed):
    r = drive([RANGE, 0], M=M, flagged=flagged)
    want = flagged if listed else None
    assert r["launches"] == [(F32, want)] and r["reads"] == 2 and r["raised"] is None
    assert r["counters"] == (0, 1, len(flagged) if listed else 0)
    assert not r["mol_err"][:M].any()
    reran, mol_list = r["out"]
    assert reran and (mol_list.tolist() == flagged if listed else mol_list is None)


def test_no_split_bit_is_kept_by_the_fp32_word():
    r = drive([RANGE, 0], prec=F16X3 | _lib.PREC_NO_SPLIT, flagged=[1])
    assert r["launches"] == [(F32 | _lib.PREC_NO_SPLIT, [1])]
    assert fp32_prec(_lib.PREC_BF16 | _lib.PREC_NO_SPLIT | _lib.EGCL_VARIANTS) == F32 | _lib.PREC_NO_SPLIT


@pytest.mark.parametrize("word", [SMALL, RANGE | SMALL])
def test_small_reruns_like_range(word):
    r = drive([word, 0], flagged=[6], bit=SMALL)
    assert r["launches"] == [(F32, [6])] and r["counters"] == (0, 1, 1) and r["raised"] is None


def test_already_fp32_raises_range_error():
    r = drive([RANGE], prec=F32, flagged=[1])
    assert r["launches"] == [] and r["reads"] == 1 and r["counters"] == (0, 0, 0)
    assert isinstance(r["raised"], _lib.RangeError)
    assert not r["mol_err"].any()                # a word that is still set: the cached words are zeroed
    assert not retry_fp32(RANGE, F32) and retry_fp32(RANGE, F16X3) and not retry_fp32(0, F16X3)


@pytest.mark.parametrize("word", [FEW, FEW | RANGE, HANDOFF | FEW])
def test_other_bits_raise_without_a_relaunch(word):
    r = drive([word], flagged=[1], hooks=True)
    assert r["launches"] == [] and r["reads"] == 1 and r["counters"] == (0, 0, 0)
    assert isinstance(r["raised"], IndexError)
    assert not r["mol_err"].any()
    assert r["log"] == [("read",), ("settle",)]


def test_handoff_alone():
    r = drive([HANDOFF, 0], flagged=[1], hooks=True)
    assert r["launches"] == [(F16X3 | _lib.PREC_NO_SPLIT, None)] and r["raised"] is None
    assert r["counters"] == (1, 0, 0) and r["out"] == (True, None)
    assert r["log"] == [("read",), ("zero_handoff",), r["log"][2], ("read",), ("settle",)]
    # zeroed before the re-launch (the fake's clean second run sets nothing)
    assert not r["mol_err"].any()


@pytest.mark.parametrize("first", [HANDOFF, HANDOFF | RANGE])
def test_handoff_then_range(first):
    r = drive([first, RANGE, 0], hooks=True)
    no_split = F16X3 | _lib.PREC_NO_SPLIT
    assert r["launches"] == [(no_split, None), (F32 | _lib.PREC_NO_SPLIT, None)]
    assert r["counters"] == (1, 1, 0) and r["raised"] is None and r["out"] == (True, None)
    assert [x[0] for x in r["log"]] == ["read", "zero_handoff", "launch", "read", "zero_fp32", "launch", "read",
                                        "settle"]
    assert r["log"][4] == ("zero_fp32", None)


def test_handoff_left_after_its_rerun_is_raised():
    r = drive([HANDOFF, HANDOFF])
    assert len(r["launches"]) == 1 and r["counters"] == (1, 0, 0)
    assert isinstance(r["raised"], _lib.HipPathError)


def test_no_per_molecule_words_reruns_the_whole_batch():
    r = drive([RANGE, 0], mol_err=False, hooks=True)
    assert r["launches"] == [(F32, None)] and r["counters"] == (0, 1, 0) and r["raised"] is None
    assert r["log"] == [("read",), ("zero_fp32", None), ("launch", F32, None), ("read",), ("settle",)]


def test_listed_molecules_reach_the_zero_hook():
    r = drive([RANGE, 0], flagged=[4], hooks=True)
    assert r["log"] == [("read",), ("zero_fp32", [4]), ("launch", F32, [4]), ("read",), ("settle",)]


def test_word_still_set_after_fp32_is_raised():
    words = [RANGE, RANGE]
    r = drive(words, flagged=[3], hooks=True)
    assert r["launches"] == [(F32, [3])] and r["reads"] == 2 and r["counters"] == (0, 1, 1)
    assert isinstance(r["raised"], _lib.RangeError)
    assert not r["mol_err"].any() and r["log"][-1] == ("settle",)
