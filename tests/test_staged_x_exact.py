"""The arithmetic rule behind the tiled step kernel's float form of a staged x (k_step_tiled, XF).

The integer form makes x_j - x_i of two window-relative fixed-point coordinates as an exact integer difference that is
converted to f32 once: float32(a - b).  The float form keeps both operands as floats and subtracts them:
float32(a) - float32(b).  For integers of magnitude <= 2^24 both operands are exact in f32, so the f32 subtraction is
the correctly rounded exact difference: the same bits, +0 for equal operands included.  One unit beyond the range an
operand is rounded when it is converted and the two forms differ, which is why the kernel enforces the range per staged
record instead of assuming it.  numpy only: no GPU."""
import numpy as np

LIM = 1 << 24


def int_form(a, b):
    """(float)(a - b): the exact difference (|a - b| <= 2^26 fits any integer type here), rounded once"""
    return (a.astype(np.int64) - b.astype(np.int64)).astype(np.float32)


def float_form(a, b):
    """(float)a - (float)b in f32"""
    return a.astype(np.float32) - b.astype(np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_random_pairs_in_the_range_give_equal_bits():
    rng = np.random.default_rng(20240611)
    for _ in range(4):
        a = rng.integers(-LIM, LIM + 1, size=5_000_000, dtype=np.int64)
        b = rng.integers(-LIM, LIM + 1, size=5_000_000, dtype=np.int64)
        assert (bits(int_form(a, b)) == bits(float_form(a, b))).all()
    # differences that need rounding (beyond 2^24 in magnitude, odd) are among them: the rule is not vacuous
    d = a - b
    assert ((np.abs(d) > LIM) & (d % 2 != 0)).any()


def test_edge_pairs_in_the_range_give_equal_bits():
    near = np.arange(-40, 41, dtype=np.int64)
    edge = np.unique(np.concatenate([near - LIM, near + LIM, near, near - LIM // 2, near + LIM // 2,
                                     near + (LIM - (1 << 23)), near - (LIM - (1 << 23))]))
    edge = edge[(edge >= -LIM) & (edge <= LIM)]
    assert -LIM in edge and LIM in edge and 0 in edge
    a, b = [m.reshape(-1) for m in np.meshgrid(edge, edge, indexing="ij")]
    want, got = int_form(a, b), float_form(a, b)
    assert (bits(want) == bits(got)).all()
    # equal operands: +0, never -0
    same = a == b
    assert same.any() and (bits(got[same]) == 0).all() and (bits(want[same]) == 0).all()
    # 2^30, where the pads and the invisible agents are staged, is exact too: the same bits against any x in the range
    far = np.full(len(edge), 1 << 30, dtype=np.int64)
    assert (bits(int_form(far, edge)) == bits(float_form(far, edge))).all()


def test_one_unit_outside_the_range_the_forms_differ():
    """2^24 + 1 is not a float: converted first it becomes 2^24, and the difference with 1 is off by one."""
    a = np.array([LIM + 1, -(LIM + 1)], dtype=np.int64)
    b = np.array([1, -1], dtype=np.int64)
    want, got = int_form(a, b), float_form(a, b)
    assert want.tolist() == [float(LIM), -float(LIM)]
    assert (bits(want) != bits(got)).all()
    # ... and over all partners in the range, for the first value beyond either end
    partners = np.arange(-LIM, LIM + 1, 4099, dtype=np.int64)
    for out in (LIM + 1, -(LIM + 1)):
        o = np.full(len(partners), out, dtype=np.int64)
        assert (bits(int_form(o, partners)) != bits(float_form(o, partners))).any()
