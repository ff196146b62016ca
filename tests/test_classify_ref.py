"""The read-out rule of glf_graph_classify (include/glf.h, "label read-out") restated twice in numpy and compared, no GPU:

  the rule text      sort the k scores: the winner is the largest score above -inf, the lowest index among equals (+0 and -0 are
                     equal, a NaN never wins), the runner-up the largest of the others from -inf, margin +0 where the two are equal
                     and best - second otherwise;
  the kernel's way   a lane holds the 16 classes j = (g & 3) + 8 (g >> 2) + 4 h of half-wave h, runs a top two over g ascending with
                     strict comparisons, exchanges the three values with the other half once and merges: the other half wins if
                     b' > b or (b' == b and l' < l), second = max(min(b, b'), max(s, s')). Slots j >= k are masked by index.

The two must agree on every table: random ones, tables of small integers (ties everywhere), and tables sprinkled with NaN, both
infinities and both zeros, for every k from 1 to 32. Two plausible but wrong merges are restated too and must be caught: one that
lets the other half win a tie whatever its index, and one that takes the runner-up from the winning half alone."""
import numpy as np
import pytest

NEG_INF = np.float32(-np.inf)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _margin(best, second):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(0.0) if best == second else np.float32(best - second)


def rule(scores):
    """(label, best, margin) of one pixel's k f32 scores, by the rule text."""
    s = np.asarray(scores, dtype=np.float32)
    above = [j for j in range(s.size) if s[j] > NEG_INF]                    # (a NaN compares false)
    if not above:
        return 0, NEG_INF, np.float32(0.0)
    order = sorted(above, key=lambda j: (-float(s[j]), j))                   # -0.0 == 0.0: equal scores fall back on the index
    label = order[0]
    best = s[label]
    second = s[order[1]] if len(order) > 1 else NEG_INF
    return label, best, _margin(best, second)


def _lane(s, k, h):
    best, label, second = NEG_INF, 0, NEG_INF
    for g in range(16):
        j = (g & 3) + 8 * (g >> 2) + 4 * h
        if j >= k:
            continue
        if s[j] > best:
            second, best, label = best, s[j], j
        elif s[j] > second:
            second = s[j]
    return best, label, second


def kernel_way(scores, merge="pinned"):
    """(label, best, margin) by the kernel's epilogue; merge: "pinned", or one of the two wrong merges."""
    s = np.asarray(scores, dtype=np.float32)
    k = s.size
    b0, l0, s0 = _lane(s, k, 0)
    b1, l1, s1 = _lane(s, k, 1)
    if merge == "other half wins ties":
        other = b1 >= b0
    else:
        other = b1 > b0 or (b1 == b0 and l1 < l0)
    if merge == "second of the winning half":
        second = s1 if other else s0
    else:
        second = max(min(b0, b1), max(s0, s1))                              # (no NaN reaches here)
    best, label = (b1, l1) if other else (b0, l0)
    return label, best, _margin(best, second)


def _same(got, want):
    return got[0] == want[0] and _bits(got[1]) == _bits(want[1]) and _bits(got[2]) == _bits(want[2])


def _tables():
    """Score tables [pixels, 32]: random, small integers, and both with specials sprinkled in."""
    rng = np.random.default_rng(5)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    smooth = rng.normal(size=(300, 32)).astype(np.float32)
    ints = rng.integers(-2, 3, size=(300, 32)).astype(np.float32)
    out = [smooth, ints]
    for base, share in ((smooth, 0.2), (ints, 0.3), (ints, 0.9)):
        t = base.copy()
        hit = rng.random(t.shape) < share
        t[hit] = specials[rng.integers(0, specials.size, int(hit.sum()))]
        out.append(t)
    hand = np.full((8, 32), np.nan, dtype=np.float32)
    hand[1, 7] = 3.0                                                         # one finite score
    hand[2] = -np.inf                                                        # nothing above -inf
    hand[3] = np.inf                                                         # every class at +inf
    hand[4] = 0.0
    hand[4, 4::8] = -0.0                                                     # zeros of both signs
    hand[5] = -0.0
    hand[5, 5] = 0.0
    hand[6, 2], hand[6, 5] = 2.0, 2.0                                        # a tie across the halves, the lower index in half 0
    hand[7, 9], hand[7, 4] = 2.0, 2.0                                        # ... the lower index in half 1
    out.append(hand)
    return np.concatenate(out)


TABLES = _tables()


@pytest.mark.parametrize("k", range(1, 33))
def test_the_epilogue_is_the_rule(k):
    for row in TABLES:
        got, want = kernel_way(row[:k]), rule(row[:k])
        assert _same(got, want), (k, row[:k], got, want)
        label, best, margin = got
        assert 0 <= label < k and not np.isnan(best) and not np.isnan(margin)
        assert _bits(margin) != _bits(np.float32(-0.0)) and margin >= 0


def test_special_cases_by_hand():
    f = np.float32
    assert _same(kernel_way([f(2.5)]), (0, f(2.5), f(np.inf)))                                   # k = 1
    assert _same(kernel_way([f(np.nan)] * 9), (0, NEG_INF, f(0.0)))                             # all NaN
    assert _same(kernel_way([f(np.nan), f(-np.inf), f(-np.inf)]), (0, NEG_INF, f(0.0)))         # nothing above -inf
    assert _same(kernel_way([f(np.nan)] * 6 + [f(-4.0)] + [f(np.nan)]), (6, f(-4.0), f(np.inf)))   # one finite score
    assert _same(kernel_way([f(1.0), f(-np.inf), f(np.nan)]), (0, f(1.0), f(np.inf)))
    assert _same(kernel_way([f(np.inf), f(1.0), f(np.inf)]), (0, f(np.inf), f(0.0)))            # two infinities: a tie, not a NaN
    assert _same(kernel_way([f(np.inf), f(1.0)]), (0, f(np.inf), f(np.inf)))
    assert _same(kernel_way([f(-0.0), f(-1.0), f(-1.0), f(-1.0), f(0.0)]), (0, f(-0.0), f(0.0)))  # +0 and -0 tie: best keeps the winner's sign
    assert _same(kernel_way([f(0.0), f(-1.0), f(-1.0), f(-1.0), f(-0.0)]), (0, f(0.0), f(0.0)))
    assert _same(kernel_way([f(1.0), f(3.0), f(2.0), f(0.0), f(3.0)]), (1, f(3.0), f(0.0)))      # the lower index wins across the halves
    assert _same(kernel_way([f(1.0), f(0.0), f(2.0), f(0.0), f(3.0), f(3.0)]), (4, f(3.0), f(0.0)))
    assert _same(kernel_way([f(5.0), f(4.0), f(1.0), f(1.0), f(2.0)]), (0, f(5.0), f(1.0)))      # the runner-up sits in the winner's half


@pytest.mark.parametrize("wrong", ["other half wins ties", "second of the winning half"])
def test_a_wrong_merge_is_caught(wrong):
    caught = 0
    for k in (5, 8, 32):
        for row in TABLES:
            caught += not _same(kernel_way(row[:k], merge=wrong), rule(row[:k]))
    assert caught > 0, wrong
    # and on the smallest tables that tell them apart
    if wrong == "other half wins ties":
        row = np.array([1, 2, 0, 0, 2], dtype=np.float32)                    # classes 1 (half 0) and 4 (half 1) tie
        assert rule(row)[0] == 1 and kernel_way(row, merge=wrong)[0] == 4
    else:
        row = np.array([5, 1, 0, 0, 4], dtype=np.float32)                    # the runner-up (class 4) sits in the other half
        assert rule(row)[2] == 1.0 and kernel_way(row, merge=wrong)[2] == 4.0
