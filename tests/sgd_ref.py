"""The momentum-SGD step of cvk_sgd_step_ranges restated in numpy, over flat arrays with a range table (no GPU, no torch).

    d = g * coef;  d = d + wd * p
    if the record uses a momentum buffer (a buffer is given and momentum != 0):
        b = d if first else momentum * buf + (1 - dampening) * d;  buf = b;  d = d + momentum * b if nesterov else b
    p_new = p - lr * d;   ema = ema + alpha * (p_new - ema)

`dtype` is the precision of EVERY operation: numpy.float64 is the reference, numpy.float32 the same expression list with one rounding per
operation (what the kernel does when the compiler contracts nothing).  The hyper-parameters are taken as given: callers pass the
float32-rounded values the kernel sees, which are exact in either precision.

Next to the values the step returns the magnitude sums S_b and S_p the tests' error bounds are relative to: the same expressions with every
term replaced by its absolute value (|1 - dampening| is formed from two exact numbers, so it stays one term)."""
import collections

import numpy as np

Record = collections.namedtuple("Record", "lr momentum dampening weight_decay nesterov first")


def record(lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first=False):
    """A record with its floats rounded to float32, as cvk_sgd_hyper_fill stores them."""
    f = lambda x: float(np.float32(x))
    return Record(f(lr), f(momentum), f(dampening), f(weight_decay), bool(nesterov), bool(first))


Step = collections.namedtuple("Step", "p buf ema S_p S_b covered used_buf")


def sgd_step(p, g, buf, ema, ranges, records, coef=1.0, alpha=None, dtype=np.float64):
    """One step.  p, g: flat arrays; buf, ema: flat arrays or None; ranges: [(offset, length, record index)]; records: [Record];
    coef: the clip coefficient (1.0 without a clip record); alpha: the EMA weight (required with ema).
    Returns Step(p, buf, ema, S_p, S_b, covered, used_buf): new arrays of `dtype` (elements outside every range are the inputs converted;
    buf / ema None stay None), the magnitude sums in float64 (0 outside the ranges; S_b 0 where no buffer is used), and boolean masks of
    the elements inside a range and of those whose momentum buffer was written."""
    T = dtype
    n = p.shape[0]
    pn, S_p, S_b = p.astype(T), np.zeros(n), np.zeros(n)
    bn = None if buf is None else buf.astype(T)
    en = None if ema is None else ema.astype(T)
    covered, used_buf = np.zeros(n, bool), np.zeros(n, bool)
    c = T(coef)
    for off, length, ri in ranges:
        r = records[ri]
        s = slice(off, off + length)
        assert 0 <= off and off + length <= n and length > 0 and not covered[s].any()
        covered[s] = True
        lr, mom, damp, wd = T(r.lr), T(r.momentum), T(r.dampening), T(r.weight_decay)
        p0, g0 = p[s].astype(T), g[s].astype(T)
        d = g0 * c
        d = d + wd * p0
        a_d = np.abs(g[s].astype(np.float64)) * abs(float(coef)) + r.weight_decay * np.abs(p[s].astype(np.float64))
        if bn is not None and r.momentum != 0.0:
            used_buf[s] = True
            if r.first:
                b, a_b = d, a_d
            else:
                b0 = buf[s].astype(T)
                b = mom * b0 + (T(1) - damp) * d
                a_b = r.momentum * np.abs(buf[s].astype(np.float64)) + abs(1.0 - r.dampening) * a_d
            bn[s] = b
            S_b[s] = a_b
            if r.nesterov:
                d, a_d = d + mom * b, a_d + r.momentum * a_b
            else:
                d, a_d = b, a_b
        new = p0 - lr * d
        pn[s] = new
        S_p[s] = np.abs(p[s].astype(np.float64)) + r.lr * a_d
        if en is not None:
            e0 = ema[s].astype(T)
            en[s] = e0 + T(alpha) * (new - e0)
    return Step(pn, bn, en, S_p, S_b, covered, used_buf)


U32 = 2.0 ** -24


def bounds(step64, ema_before=None, alpha=None):
    """The element-wise error bounds of an fp32 evaluation against `step64` (the float64 Step): 5 roundings on the longest path from g to b
    and 9 to p_new (FMA contraction only removes roundings), so 6 u S_b and 10 u S_p; the EMA makes two more on top of p_new:
    12 u (|ema| + alpha (S_p + |ema|)) with ema the value before the step."""
    bb, bp = 6 * U32 * step64.S_b, 10 * U32 * step64.S_p
    be = None
    if ema_before is not None:
        e = np.abs(ema_before.astype(np.float64))
        be = 12 * U32 * (e + float(alpha) * (step64.S_p + e))
    return bp, bb, be


# ---- the kernel-level case that tests/test_gpu_sgd.py runs on the GPU and tests/test_sgd_cpu.py runs on the reference alone -----------------
CASE_N = 5003                                    # not a multiple of 4
# (offset, length, record): the first range starts after a gap at offset 0 and is longer than its workgroups' stride (256 * 3 + 5 elements for
# the two workgroups CASE_BLOCK0 gives it: the first workgroup's threads and five of the second's make a second trip); one of length 1; one
# that ends at n
CASE_RANGES = [(5, 256 * 3 + 5, 1), (1000, 1, 0), (2000, 1500, 2), (4800, 203, 0)]
CASE_BLOCK0 = [0, 2, 3, 9]                       # 2, 1, 6 and 1 workgroups of 256 threads
CASE_BLOCKS = 10
CASE_CLIP = (3.0, 0.37)                          # {total_norm, clip_coef}
CASE_ALPHA = 0.1
NAN_BITS = 0x7FC00ABC                            # a NaN with a payload: everything outside the ranges


def case_records(mom):
    """first = 1; first = 0 with Nesterov; first = 0 with dampening 0.3 and weight decay.  Without a momentum buffer the same records with
    momentum 0 (and no Nesterov, which needs one): first and dampening are then ignored, as torch ignores them."""
    if mom:
        return [record(0.05, 0.9, 0.0, 1e-2, False, True), record(0.03, 0.9, 0.0, 0.0, True, False), record(0.07, 0.8, 0.3, 1e-2, False, False)]
    return [record(0.05, 0.0, 0.0, 1e-2, False, True), record(0.03, 0.0, 0.0, 0.0, False, False), record(0.07, 0.0, 0.3, 1e-2, False, False)]


def case_inputs():
    """(p, g, buf, ema) float32: magnitudes spread over 1e-4 ... 1e2, both signs, from a seeded generator; p, buf and ema hold NAN_BITS
    outside the ranges (g holds numbers there: it is only read, and must not be read there either)."""
    rng = np.random.default_rng(2024)
    arrs = [(10.0 ** rng.uniform(-4, 2, CASE_N) * rng.choice([-1.0, 1.0], CASE_N)).astype(np.float32) for _ in range(4)]
    inside = np.zeros(CASE_N, bool)
    for o, m, _ in CASE_RANGES:
        inside[o:o + m] = True
    for a in (arrs[0], arrs[2], arrs[3]):
        a.view(np.uint32)[~inside] = NAN_BITS
    return arrs


def check_case(got_p, got_buf, got_ema, clip, ema, mom, what):
    """Assert the results of one step of the case (float32 arrays; got_buf / got_ema None where the case has none) against the float64
    reference: every element inside a range within the derived bounds, everything else bitwise what it was.  Prints the worst ratios."""
    p, g, buf, e = case_inputs()
    coef = float(np.float32(CASE_CLIP[1])) if clip else 1.0
    alpha = float(np.float32(CASE_ALPHA)) if ema else None
    want = sgd_step(p, g, buf if mom else None, e if ema else None, CASE_RANGES, case_records(mom), coef, alpha)
    bp, bb, be = bounds(want, e if ema else None, alpha)
    c = want.covered
    assert int(c.sum()) == sum(m for _, m, _ in CASE_RANGES)
    err = np.abs(got_p[c].astype(np.float64) - want.p[c])
    print(f"{what}: worst |p - p64| / (10 u S_p) = {float((err / bp[c]).max()):.3f}")
    assert np.all(err <= bp[c]), what
    assert np.array_equal(got_p.view(np.uint32)[~c], p.view(np.uint32)[~c]), what
    if mom:
        assert np.array_equal(want.used_buf, c)
        errb = np.abs(got_buf[c].astype(np.float64) - want.buf[c])
        print(f"{what}: worst |b - b64| / (6 u S_b) = {float((errb / bb[c]).max()):.3f}")
        assert np.all(errb <= bb[c]), what
        assert np.array_equal(got_buf.view(np.uint32)[~c], buf.view(np.uint32)[~c]), what
    elif got_buf is not None:
        assert np.array_equal(got_buf.view(np.uint32), buf.view(np.uint32)), what          # the whole buffer, bit for bit
    if ema:
        erre = np.abs(got_ema[c].astype(np.float64) - want.ema[c])
        print(f"{what}: worst |ema - ema64| / bound = {float((erre / be[c]).max()):.3f}")
        assert np.all(erre <= be[c]), what
        assert np.array_equal(got_ema.view(np.uint32)[~c], e.view(np.uint32)[~c]), what
    elif got_ema is not None:
        assert np.array_equal(got_ema.view(np.uint32), e.view(np.uint32)), what
    assert not np.array_equal(got_p[c], p[c])
