"""The two division helpers of rt_dmath.h that replace the compiler's full IEEE expansion on the hot path.

div_const<ByPi>(x) is x / PI_32 as an estimate and one FMA correction.  Whether one correction always lands
on the correctly rounded quotient depends on the constant, so the claim is an enumeration: all 2^32 inputs
on the device (rt_debug_verify_div_pi), and here, without a GPU, the same recipe in exact arithmetic over a
strided 2^24 of them, so that a wrong constant or a wrong range fails before any GPU sees it.

div3_by(n, d) runs the expansion's own FMA chain without its scaling and fix-up instructions, inside the
range where those do nothing.  Identical by construction; the device comparison against plain `/`
(rt_debug_verify_div3) is the safeguard: random sets and every pairing of the values where the range test, the
scaling or the fix-up would matter.

Every comparison is bitwise (NaNs equal as NaNs).  No tolerance.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI_32 = np.float32(3.14159265359)
LO, HI = np.float32(2.0**-100), np.float32(3.402823466e+38)        # div_const's range: |x| in [LO, HI]
DIV3_LO, DIV3_HI = 2.0**-46, 2.0**46


def header_constant():
    """ByPi::C as rt_dmath.h spells it."""
    text = open(os.path.join(ROOT, "buas-pathtracer_amd", "csrc", "rt_dmath.h")).read()
    m = re.search(r"struct ByPi \{.*?C = (0x[0-9a-fA-F.]+p[-+]?\d+)f;", text, flags=re.S)
    assert m, "ByPi::C not found in rt_dmath.h"
    c = float.fromhex(m.group(1))
    assert np.float32(c) == c, "ByPi::C is no float32"
    return np.float32(c)


def fma32(a, b, c):
    """fmaf on float32 arrays, exactly: the product is exact in float64, the sum is rounded to odd there (TwoSum
    gives its error), and 53 bits are more than 2*24 + 2, so the final rounding to float32 is the single
    rounding of the exact a*b + c."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0.0) & even & np.isfinite(s)
    toward = np.where((e > 0.0), np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def test_fma32_is_fmaf():
    """The emulation against libm's fmaf on operands shaped like the recipe's (a residual of two nearly equal
    terms) and on random ones."""
    libm = C.CDLL("libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    rng = np.random.default_rng(3)
    x = rng.uniform(-4.0, 4.0, 3000).astype(np.float32)
    q = (x * np.float32(0.3183099)).astype(np.float32)
    cases = [(np.full_like(x, -PI_32), q, x), (x, q, rng.uniform(-1, 1, 3000).astype(np.float32)),
             (x * np.float32(1e-30), q * np.float32(1e-9), x * np.float32(1e-39))]
    for a, b, c in cases:
        want = np.array([libm.fmaf(float(u), float(v), float(w)) for u, v, w in zip(a, b, c)], np.float32)
        assert np.array_equal(fma32(a, b, c).view(np.uint32), want.view(np.uint32))


def test_div_pi_recipe_on_a_strided_subset():
    """q0 = x*c; q = fma(fma(-PI, q0, x), c, q0) equals x / PI_32 bit for bit for 2^24 inputs spread over all
    2^32 bit patterns (stride 257: every exponent, both signs, all low mantissa bits), wherever |x| is in the
    helper's range; c is read from the header and must be the rounded reciprocal."""
    c = header_constant()
    assert c == np.float32(1.0) / PI_32
    bad = 0
    checked = 0
    first = None
    with np.errstate(all="ignore"):
        for k in range(16):
            i = np.arange(k << 20, (k + 1) << 20, dtype=np.uint64)
            x = ((i * np.uint64(257)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
            a = np.abs(x)
            x = x[(a >= LO) & (a <= HI)]
            q0 = x * c
            q = fma32(fma32(np.full_like(x, -PI_32), q0, x), np.full_like(x, c), q0)
            want = x / PI_32
            diff = q.view(np.uint32) != want.view(np.uint32)
            checked += len(x)
            bad += int(diff.sum())
            if first is None and diff.any():
                first = hex(int(x.view(np.uint32)[np.argmax(diff)]))
    assert checked > 12_000_000
    assert bad == 0, f"{bad} of {checked} inputs differ, first at bits {first}"


def test_div_pi_range_limits_are_needed():
    """Just outside the range the recipe does differ (-0, a residual that leaves the normal range), so the range
    test is no decoration; the device helper divides there."""
    c = header_constant()
    x = np.array([-0.0], np.float32)
    with np.errstate(all="ignore"):
        q0 = x * c
        q = fma32(fma32(np.full_like(x, -PI_32), q0, x), np.full_like(x, c), q0)
    assert q.view(np.uint32)[0] != (x / PI_32).view(np.uint32)[0]


@pytest.mark.gpu
def test_div_pi_exhaustive(rt):
    """div_const<ByPi> against the IEEE division on the device: all 2^32 inputs, 0 mismatches."""
    from parity_report import REPORT
    bad, first = C.c_uint64(), C.c_uint32()
    assert rt.lib().rt_debug_verify_div_pi(0, C.byref(bad), C.byref(first)) == 0
    REPORT["div_pi_exhaustive"] = {"inputs": 1 << 32, "mismatches": bad.value}
    assert bad.value == 0, f"first mismatch at bits 0x{first.value:08x}"


def edge_values():
    f = np.float32
    up = lambda v: np.nextafter(f(v), f(np.inf))
    dn = lambda v: np.nextafter(f(v), f(-np.inf))
    pos = [0.0, 1e-45, 1.1754942e-38, 2.0**-126, 2.0**-103, dn(2.0**-103), up(2.0**-103),
           DIV3_LO, dn(DIV3_LO), up(DIV3_LO), DIV3_HI, dn(DIV3_HI), up(DIV3_HI),
           2.0**-23, 0.01, 1.0, dn(1.0), up(1.0), dn(2.0), 3.0, 1.0 / 3.0, 2.0**96, 2.0**126, up(2.0**126),
           3.402823466e+38, np.inf]
    pos += [np.array([0x3F7FFFFF, 0x40FFFFFF, 0x28FFFFFF, 0x56FFFFFF], np.uint32).view(f)[i] for i in range(4)]  # mantissas of all ones
    v = np.array([f(p) for p in pos], f)
    return np.concatenate([v, -v, np.array([np.nan], f)])


def div3_mismatches(rt, sets):
    sets = np.ascontiguousarray(sets, np.float32)
    assert sets.ndim == 2 and sets.shape[1] == 4
    bad, first = C.c_uint64(), C.c_uint32()
    code = rt.lib().rt_debug_verify_div3(0, len(sets), sets.ctypes.data_as(C.POINTER(C.c_float)), C.byref(bad),
                                         C.byref(first))
    assert code == 0
    return bad.value, first.value


@pytest.mark.gpu
def test_div3_random_sets(rt):
    """2^20 seeded (numerator triple, denominator) sets: a quarter of them any bit pattern (mostly out of range:
    the plain divisions), the rest with exponents around the range and its limits, so that sets wholly inside,
    wholly outside and straddling it all occur."""
    from parity_report import REPORT
    rng = np.random.default_rng(20)
    n = 1 << 20
    bits = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    near = np.arange(n) >= n // 4
    e = rng.integers(127 - 50, 127 + 51, (n, 4), dtype=np.uint64).astype(np.uint32)
    bits[near] = (bits[near] & np.uint32(0x807FFFFF)) | (e[near] << np.uint32(23))
    sets = bits.view(np.float32)
    a = np.abs(sets)
    inside = np.all((a >= DIV3_LO) & (a <= DIV3_HI), axis=1)
    assert 0.3 < inside.mean() < 0.95 and (~inside[near]).sum() > 1000
    bad, first = div3_mismatches(rt, sets)
    REPORT["div3_random"] = {"sets": n, "in_range": int(inside.sum()), "mismatches": bad}
    assert bad == 0, f"{bad} sets differ, first {sets[first].tolist() if first < n else first}"


@pytest.mark.gpu
def test_div3_edge_table(rt):
    """Every (numerator, denominator) pair of the edge values -- zeros of both signs, denormals, the range limits
    and their neighbours, the limits of the instructions' own scaling (2^-103, 2^126, 2^96), infinities, NaN,
    equal operands, mantissas of all ones -- with the other two numerators in range, on an edge value, and
    equal to the first."""
    from parity_report import REPORT
    v = edge_values()
    nn, dd = np.meshgrid(v, v, indexing="ij")
    nn, dd = nn.ravel(), dd.ravel()
    k = np.arange(len(nn))
    other = v[(k * 7 + 3) % len(v)]
    sets = np.concatenate([
        np.stack([nn, np.full_like(nn, 0.75), np.full_like(nn, -1.5), dd], 1),
        np.stack([np.full_like(nn, 0.75), nn, other, dd], 1),
        np.stack([other, np.full_like(nn, -1.5), nn, dd], 1),
        np.stack([nn, nn, nn, dd], 1)])
    bad, first = div3_mismatches(rt, sets)
    REPORT["div3_edges"] = {"sets": len(sets), "values": len(v), "mismatches": bad}
    assert bad == 0, f"{bad} sets differ, first {sets[first].tolist() if first < len(sets) else first}"
