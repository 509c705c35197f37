"""The rule behind the tiled step kernel's split time-to-collision pass (ttc_skip_key, cs_device_types.hip.inc; DESIGN.md
section 4): a pair is not finished only if  disc < 0  or  disc == 0 and bh == 0,  and for exactly these the full quadratic
(ttc_core_c_f32) returns +inf WHATEVER the hardware's 1-ulp square root and reciprocal return.

This file restates ttc_core_c_f32 in numpy f32 (fma with one rounding), with `root` and `ia` replaced by adversaries:
the correctly rounded value, one ulp either side of it, for `ia` also +inf (a reciprocal that overflows or flushes), and
for `root` the value of an instruction that flushes a denormal argument to a zero of its sign.  A NaN stays a NaN and an
exact zero stays a zero: an error of one ulp is a relative one.  The kernel's test is restated bit for bit: the sign bit
of  bits(disc + |bh|) - 1.  numpy only: no GPU."""
import numpy as np

F = np.float32
INF = F(np.inf)
DMIN = F(1.401298464324817e-45)  # smallest denormal
UNITS = 2.0 ** 22               # fixed units per metre at a cell of 2 m


def fma(a, b, c):
    """round_f32(a * b + c) with ONE rounding: the product of two f32 is exact in f64; the f64 sum is rounded to odd
    (TwoSum gives its error) before the cast, which makes the double rounding harmless (53 >= 24 + 2 bits)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
    toward = np.where(e > 0.0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    with np.errstate(over="ignore"):
        return s.astype(F)


def discriminant(rvx, rvy, rpx, rpy, c):
    """a, bh, disc as ttc_core_c_f32 and ttc_skip_key form them"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = fma(rvx, rvx, rvy * rvy)
        bh = fma(rvx, rpx, rvy * rpy)
        disc = fma(bh, bh, -(a * c))
    return a, bh, disc


def skipped(disc, bh):
    """the kernel's bit: sign of bits(disc + |bh|) - 1"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = (disc + np.abs(bh)).astype(F)
    return ((s.view(np.uint32) - np.uint32(1)) >> np.uint32(31)).astype(bool)


def one_ulp(x):
    """x and its neighbours one ulp away in magnitude; zeros, infinities and NaNs stay what they are"""
    keep = ~np.isfinite(x) | (x == 0.0)
    with np.errstate(invalid="ignore"):
        up = np.where(keep, x, np.nextafter(x, np.where(x > 0, INF, -INF).astype(F)))
        dn = np.where(keep, x, np.nextafter(x, F(0.0)))
    return [x, up.astype(F), dn.astype(F)]


def ttc_select(t0, t1):
    with np.errstate(invalid="ignore"):
        t = np.fmax(t0, F(0.0))
        t = np.where(~((t0 < 0.0) | (t0 > 0.0)), t1, t)
        return np.where(t1 > 0.0, t, INF).astype(F)


def results(a, bh, disc, flush=False):
    """ttc_core_c_f32's result for every pair of adversarial root and reciprocal: a list of arrays"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        roots = one_ulp(np.sqrt(disc.astype(np.float64)).astype(F))
        if flush:  # an instruction that reads a denormal as a zero of its sign: sqrt(+-0) = +-0
            tiny = np.abs(disc) < F(2.0 ** -126)
            roots.append(np.where(tiny, np.copysign(F(0.0), disc), roots[0]).astype(F))
        ias = one_ulp((1.0 / a.astype(np.float64)).astype(F)) + [np.where(np.isnan(a), a, INF).astype(F)]
        out = []
        for root in roots:
            for ia in ias:
                out.append(ttc_select(((-bh - root) * ia).astype(F), ((-bh + root) * ia).astype(F)))
    return out


def kernel_like_sample(n, seed):
    """quintuples as the kernel has them: integer relative positions in fixed units, c = d2 - R2, velocities of every size"""
    rng = np.random.default_rng(seed)

    def vel():
        mag = np.exp2(rng.uniform(-70.0, 45.0, n))
        v = (mag * rng.choice([-1.0, 1.0], n)).astype(F)
        walk = (rng.integers(-3, 4, n) * 0.65).astype(F)                    # a few exact, shared values: equal velocities
        pick = rng.random(n)
        return np.where(pick < 0.25, walk, np.where(pick < 0.6, (rng.normal(0.0, 1.0, n)).astype(F), v)).astype(F)
    vix, viy, vjx, vjy = vel(), vel(), vel(), vel()
    same = rng.random(n) < 0.15                                             # the neighbour walks exactly as the agent does
    vjx, vjy = np.where(same, vix, vjx), np.where(same, viy, vjy)
    with np.errstate(over="ignore", invalid="ignore"):
        rvx, rvy = (vjx - vix).astype(F), (vjy - viy).astype(F)
    reach = np.where(rng.random(n) < 0.5, 2.0 * UNITS, 2.0 ** 25)
    rpx = np.rint(rng.uniform(-1.0, 1.0, n) * reach).astype(F)
    rpy = np.rint(rng.uniform(-1.0, 1.0, n) * reach).astype(F)
    Rs = (rng.uniform(0.05, 1.0, n).astype(F) * F(UNITS)).astype(F)
    d2 = fma(rpx, rpx, rpy * rpy)
    c = (d2 - Rs * Rs).astype(F)
    return rvx, rvy, rpx, rpy, c


def test_skipped_pairs_of_a_random_sample_are_infinite_for_any_root_and_reciprocal():
    q = kernel_like_sample(1_000_000, 20241021)
    a, bh, disc = discriminant(*q)
    skip = skipped(disc, bh)
    on_set = (disc < 0.0) | ((disc == 0.0) & (bh == 0.0))
    print(f"skipped {skip.mean():.3f}, on the skip set {on_set.mean():.3f}, both zero {((disc == 0) & (bh == 0)).mean():.3f}, "
          f"negative but finished {(on_set & ~skip).sum()}, NaN discriminants {np.isnan(disc).sum()}")
    assert skip.mean() > 0.2 and (~skip).mean() > 0.05 and ((disc == 0.0) & (bh == 0.0)).mean() > 0.05
    # the bit is set only on the set (a NaN discriminant goes by its sign; its root is a NaN like a negative one's)
    assert (on_set | np.isnan(disc))[skip].all()
    for r in results(a[skip], bh[skip], disc[skip], flush=True):
        assert (r == INF).all()
    # the test is close to exact on such operands: a negative discriminant within |bh| of zero is rare
    assert (on_set & ~skip).mean() < 0.01
    # and the restatement is not vacuous: finished pairs do have finite times
    live = results(a[~skip], bh[~skip], disc[~skip])[0]
    assert np.isfinite(live).mean() > 0.1


def edge_quintuples():
    f = lambda *v: np.array(v, dtype=F)  # noqa: E731
    rows = [
        # rvx, rvy, rpx, rpy, c
        (0.0, 0.0, 3.0, -4.0, 9.0),             # a = 0, bh = 0: equal velocities
        (0.0, -0.0, -3.0, 4.0, -9.0),           # the same, overlapping, a -0 among the products
        (1e-30, 0.0, 5.0, 0.0, 9.0),            # a = 0 (underflow), bh != 0, bh^2 underflows: disc = 0
        (-1e-30, 0.0, 5.0, 0.0, 9.0),
        (1e-22, 0.0, 5.0, 0.0, 9.0),            # a denormal
        (1.0, 0.0, 7.0, 0.0, 0.0),              # c = 0: touching at R, disc = bh^2
        (0.0, 1.0, 7.0, 0.0, 0.0),              # c = 0 and bh = 0: disc = 0
        (1.0, 0.0, 1.0, 0.0, -3.0),             # c < 0: disc > 0
        (0.0, 0.0, 1.0, 0.0, -3.0),             # c < 0 with equal velocities
        (1e-40, 0.0, 3.0, 0.0, 5.0),            # rv denormal
        (1e-40, -1e-42, -3.0, 2.0, -5.0),
        (1.4e-45, 0.0, 1.0, 0.0, 1.0),
        (2.0 ** -74, 0.0, 1.0, 0.0, 3.0),       # disc = -2^-147: a negative denormal beside a normal bh
        (2.0 ** -74, 0.0, 0.0, 1.0, 3.0),       # the same with bh = 0
        (0.0, 1.0, 2.0 ** 20, 2.0 ** 22, 2.0 ** 44),   # grazing: bh^2 == a c exactly, bh != 0
        (0.0, 2.0, 8.0, 1.0, 60.0),             # a miss: disc < 0
        (3e38, 3e38, 2.0 ** 25, 2.0 ** 25, 1.0),       # everything overflows: disc = inf - inf
    ]
    return [f(*col) for col in zip(*rows)]


def test_hand_made_edges():
    q = edge_quintuples()
    a, bh, disc = discriminant(*q)
    skip = skipped(disc, bh)
    on_set = (disc < 0.0) | ((disc == 0.0) & (bh == 0.0))
    want = [True, True, False, False, False, False, True, False, True, False, False, False, False, True, False, True]
    assert skip[:16].tolist() == want, (skip.tolist(), disc.tolist(), bh.tolist())
    assert np.isnan(disc[16])  # (goes by the NaN's sign, either way)
    assert (a[[0, 2, 3]] == 0.0).all() and (bh[[2, 3]] != 0.0).all() and (disc[[2, 3]] == 0.0).all()
    assert disc[12] < 0.0 and abs(disc[12]) < 2.0 ** -126 and not skip[12]   # conservative: finished
    assert disc[14] == 0.0 and bh[14] == 2.0 ** 22
    assert (on_set | np.isnan(disc))[skip].all()
    for r in results(a[skip], bh[skip], disc[skip], flush=True):
        assert (r == INF).all()
    # the grazing pair is worth finishing: it touches after 2^22 units of time
    assert results(a[14:15], -bh[14:15], disc[14:15])[0][0] == 2.0 ** 22


def test_the_bit_on_special_values_of_disc_and_bh():
    """every pair of special values: the bit is set only on the set, and wherever it is set the result is +inf for every
    a.  (No flushing root here: a negative denormal discriminant beside a smaller non-zero denormal bh would be marked
    and could come out finite from such a root.  The kernel's operands cannot get there: relative positions are
    integers, so a non-zero |bh| below 2^-126 needs |rv| below 2^-102, whose a = |rv|^2 underflows to 0 and takes the
    discriminant to +-0 with it.  The sample above, which has such velocities, runs with the flushing root.)"""
    big = F(3.4028234663852886e38)
    sp = np.array([0.0, -0.0, DMIN, -DMIN, 2.0 ** -126, -(2.0 ** -126), 1.0, -1.0, 1.0 + 2.0 ** -23, big, -big, np.inf, -np.inf,
                   np.nan, -np.nan, 2.0 ** -127, -(2.0 ** -127), 2.0 ** 22, -(2.0 ** 22)], dtype=F)
    sp = np.concatenate([sp, np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001], dtype=np.uint32).view(F)])
    disc, bh, a = [m.reshape(-1) for m in np.meshgrid(sp, sp, sp, indexing="ij")]
    skip = skipped(disc, bh)
    on_set = (disc < 0.0) | ((disc == 0.0) & (bh == 0.0))
    nan_result = np.isnan(disc) | (np.isinf(disc) & np.isinf(bh))  # disc + |bh| is a NaN: goes by the sign it carries
    assert (on_set | nan_result)[skip].all()
    assert skip[on_set & (disc < -np.abs(bh))].all() and skip[(disc == 0.0) & (bh == 0.0) & ~np.signbit(disc)].all()
    for r in results(a[skip], bh[skip], disc[skip]):
        assert (r == INF).all()


def test_just_off_the_set_is_finished():
    z, d = F(0.0), DMIN
    disc = np.array([d, d, d, z, z, -z, z], dtype=F)
    bh = np.array([z, F(1.0), -d, d, -d, d, F(-1.0)], dtype=F)
    assert not skipped(disc, bh).any()
    # and on it (a discriminant of -0 beside bh = 0 included: -0 + |bh| is +0)
    disc = np.array([-d, z, z, -z, F(-1.0), -INF], dtype=F)
    bh = np.array([z, z, -z, z, F(0.5), F(3.0)], dtype=F)
    assert skipped(disc, bh).all()
