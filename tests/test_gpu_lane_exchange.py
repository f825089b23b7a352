"""lane_exchange<S> (fast-racing_amd/csrc/frx_wave.hpp): the neighbour exchange of one step of the lane = knot reductions in the one-launch evaluation - wave-shift DPP
moves for S = 1 and 2, v_permlane16_swap / v_permlane32_swap for S = 16 and 32, the shuffles for 4 and 8.  One wave through frx_debug_lane_exchange:
below[i] = in[i - S], above[i] = in[i + S], compared with array slicing as raw 64-bit patterns - the exchange moves the two halves of a double and must not touch them:
NaNs keep their payloads and stay signalling, -0.0 keeps its sign, subnormals are not flushed.  A lane without a source lane may hold anything and is not compared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIDES = (1, 2, 4, 8, 16, 32)


def _patterns():
    """name -> 64 words.  Every word of a set differs from every other one, so a lane that took the wrong source shows."""
    lane = np.arange(64, dtype=np.uint64)
    rng = np.random.default_rng(20240611)
    p = {}
    p["lane_numbers"] = (lane + np.uint64(1)) * np.uint64(0x0101010101010101) ^ (lane << np.uint64(32))
    p["halves_differ"] = (lane << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - lane)                      # a swapped or doubled half shows
    p["random_bits"] = rng.integers(0, 2**64, size=64, dtype=np.uint64)
    p["quiet_nans_with_payloads"] = np.uint64(0x7FF8000000000000) | (lane + np.uint64(1)) | ((lane & np.uint64(1)) << np.uint64(63))
    p["signalling_nans_with_payloads"] = np.uint64(0x7FF0000000000000) | ((lane + np.uint64(1)) << np.uint64(20)) | (lane + np.uint64(1))
    p["subnormals"] = (lane + np.uint64(1)) | ((lane & np.uint64(1)) << np.uint64(63))                  # +-(lane + 1) 2^-1074
    special = np.array([0x8000000000000000, 0x0000000000000000, 0xFFFFFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF,
                        0x7FEFFFFFFFFFFFFF], dtype=np.uint64)                                           # -0.0, +0.0, all ones, +-inf, the smallest and the largest subnormal, the largest finite
    p["special_values"] = np.concatenate([special, rng.integers(0, 2**64, size=56, dtype=np.uint64)])
    p["special_values_in_every_row"] = np.tile(np.concatenate([special, special ^ np.uint64(0x0000000100000000)]), 4) ^ (lane >> np.uint64(4)) << np.uint64(8)
    p["all_ones_everywhere"] = np.full(64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    p["minus_zero_everywhere"] = np.full(64, 0x8000000000000000, dtype=np.uint64)
    return p


PATTERNS = _patterns()


def test_the_patterns_are_the_ones_meant():
    for name in ("lane_numbers", "halves_differ", "random_bits", "quiet_nans_with_payloads", "signalling_nans_with_payloads", "subnormals", "special_values"):
        assert np.unique(PATTERNS[name]).size == 64, name
    as_f = lambda n: PATTERNS[n].view(np.float64)
    assert np.all(np.isnan(as_f("quiet_nans_with_payloads"))) and np.all(np.isnan(as_f("signalling_nans_with_payloads"))) and np.all(np.isnan(as_f("all_ones_everywhere")))
    assert np.all((PATTERNS["signalling_nans_with_payloads"] & np.uint64(0x0008000000000000)) == 0)     # the quiet bit is clear
    sub = as_f("subnormals")
    assert np.all(sub != 0.0) and np.all(np.abs(sub) < np.finfo(np.float64).tiny)
    assert np.all(as_f("minus_zero_everywhere") == 0.0) and np.all(np.signbit(as_f("minus_zero_everywhere")))
    assert PATTERNS["special_values"][0] == 0x8000000000000000 and PATTERNS["special_values"][2] == 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("name", list(PATTERNS))
@pytest.mark.parametrize("stride", STRIDES)
def test_exchange_against_slicing(frx, stride, name):
    v = PATTERNS[name]
    below, above = frx.lane_exchange(stride, v)
    assert below.dtype == np.uint64 and above.dtype == np.uint64
    bad_b = np.flatnonzero(below[stride:] != v[:64 - stride]) + stride
    bad_a = np.flatnonzero(above[:64 - stride] != v[stride:])
    assert bad_b.size == 0, (stride, name, "from below", [(int(i), hex(int(below[i])), hex(int(v[i - stride]))) for i in bad_b[:4]])
    assert bad_a.size == 0, (stride, name, "from above", [(int(i), hex(int(above[i])), hex(int(v[i + stride]))) for i in bad_a[:4]])


def test_a_stride_outside_the_six_is_refused(frx):
    for stride in (0, 3, 64, -1):
        with pytest.raises(frx.FrxError):
            frx.lane_exchange(stride, PATTERNS["lane_numbers"])
