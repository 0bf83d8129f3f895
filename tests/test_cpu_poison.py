"""The poisoned-buffer helper (tests/_poison.py) on the CPU: its checks fail on
a flipped guard byte, an unwritten output element and a changed input, pass
otherwise, place regions at the alignments asked for, and every fit case of
tests/test_gpu_buffers.py has a positive workspace size (the planning code of
csrc/fit_plan.hpp needs no GPU)."""

import numpy as np
import pytest

import _poison as P


def _arena():
    A = P.Arena()
    A.add("X", 7 * 24, 16, 8).add("codes", 13, 1).add("out", 5 * 8).add("st", 3 * 4).add("ws", 1000)
    A.build()
    A.put("X", np.arange(21, dtype=np.float64))
    A.put("codes", np.arange(13, dtype=np.uint8))
    return A


def _write_outputs(A):
    A.buf[A.regions["out"][0]:][:40] = np.linspace(0.0, 1.0, 5).view(np.uint8)
    A.buf[A.regions["st"][0]:][:12] = np.array([0, 3, 4], np.int32).view(np.uint8)


def test_layout_alignment_and_guards():
    A = _arena()
    assert A.ptr("X") % 16 == 8 and A.ptr("out") % 256 == 0 and A.ptr("ws") % 256 == 0
    spans = sorted(A.regions.values())
    assert spans[0][0] >= P.GUARD
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o1 - (o0 + n0) >= P.GUARD
    assert A.buf.size - (spans[-1][0] + spans[-1][1]) >= P.GUARD
    assert np.array_equal(A.get("X", np.float64), np.arange(21.0))
    assert (A.raw("ws") == 0xFF).all() and np.isnan(A.get("out", np.float64)).all()
    assert (A.get("st", np.int32) == -1).all()


def test_checks_pass_on_a_clean_call():
    A = _arena()
    _write_outputs(A)
    A.fill("ws", 0x5A)
    assert A.guards_intact() and A.inputs_unchanged()
    assert A.fully_written("out", np.float64) and A.fully_written("st", np.int32)


@pytest.mark.parametrize("where", ["before_first", "after_X", "before_out", "after_ws", "last_byte"])
def test_one_flipped_guard_byte_fails(where):
    A = _arena()
    _write_outputs(A)
    at = {"before_first": 0, "after_X": sum(A.regions["X"]),
          "before_out": A.regions["out"][0] - 1, "after_ws": sum(A.regions["ws"]),
          "last_byte": A.buf.size - 1}[where]
    assert A.buf[at] == 0xFF
    A.buf[at] = 0xFE
    with pytest.raises(AssertionError, match="guard byte changed"):
        A.guards_intact()
    A.buf[at] = 0xFF
    assert A.guards_intact()


@pytest.mark.parametrize("name,dtype,index", [("out", np.float64, 0), ("out", np.float64, 4),
                                              ("st", np.int32, 1)])
def test_one_unwritten_output_element_fails(name, dtype, index):
    A = _arena()
    _write_outputs(A)
    size = np.dtype(dtype).itemsize
    off = A.regions[name][0] + index * size
    A.buf[off:off + size] = 0xFF
    with pytest.raises(AssertionError, match=f"'{name}'.*index {index}"):
        A.fully_written(name, dtype)
    A.buf[off] = 0xFE  # a NaN with another payload was written by somebody
    assert A.fully_written(name, dtype)


def test_a_written_input_fails():
    A = _arena()
    A.buf[A.regions["codes"][0] + 5] ^= 1
    with pytest.raises(AssertionError, match="'codes'"):
        A.inputs_unchanged()


def test_stale_image_is_repeated_to_length():
    A = _arena()
    A.put_bytes("ws", np.arange(7, dtype=np.uint8))
    assert np.array_equal(A.raw("ws"), np.tile(np.arange(7, dtype=np.uint8), 143)[:1000])
    assert A.guards_intact() and A.inputs_unchanged()


def test_zero_block_and_bit_equality_helpers():
    out = dict(theta=np.zeros((2, 3)), sig_inv=np.zeros((2, 3, 3)), sig_inv_theta=np.zeros((2, 3)),
               loglik=np.zeros(2), iters=np.zeros(2, np.int32))
    P.check_zero_blocks(out, [P.STATUS_EMPTY, P.STATUS_NONFINITE])
    out["sig_inv"][1, 2, 2] = np.nan
    P.check_zero_blocks(out, [P.STATUS_EMPTY, P.STATUS_OK])
    with pytest.raises(AssertionError):
        P.check_zero_blocks(out, [P.STATUS_EMPTY, P.STATUS_SINGULAR])
    assert P.bits_equal(np.array([np.nan, 0.0]), np.array([np.nan, 0.0]))
    assert not P.bits_equal(np.array([0.0]), np.array([-0.0]))


@pytest.mark.parametrize("case", P.FIT_CASES + [P.STALE_POISSON, P.STALE_LOGISTIC, P.SKEW_CASE],
                         ids=P.FIT_CASE_IDS + ["stale-poisson", "stale-logistic", "wide-skewed"])
def test_workspace_size_of_every_fit_case(case):
    from dlsa_amd import _hip

    need = P.workspace_bytes(_hip.load(), case)
    assert need > 0 and need % 256 == 0
    assert case.K == len(case.sizes) and case.offsets[-1] == sum(case.sizes) > 0
    assert (case.P > _hip.MAX_P_FUSED) == ("wide" in case.id)  # the path the id names
