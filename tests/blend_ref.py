"""The reference of the blend read-out's epilogue (glf_graph_blend, include/glf.h), in numpy float32, from a table of scores.

emulate() restates what k_graph_blend does after its scores exist, step by step:
  1. ownership: register g of the lanes of half-wave h holds slot acc_row(g, h) = (g & 3) + 8 (g >> 2) + 4 h of a pixel (slot s lives
     in half (s >> 2) & 1); the table [slots, N] is dealt to regs [2, 16, N] by that rule and written back as the wave's
     [pixel][slot] image by the same rule -- a kernel that files a register under the other half-wave's slot swaps slots s and s ^ 4;
  2. the index rule, in float32: tc = fminf(fmaxf(t, 0), nlevels - 1) (a NaN level reads as 0), i = min((int)tc, nlevels - 2),
     f = tc - (float)i, and per output o: lo = o nlevels + i, hi = lo + 1;
  3. the read-out: out = f == 0 ? z_lo : f == 1 ? z_hi : fmaf(f, z_hi, fmaf(-f, z_lo, z_lo)), with edges_ref.fmaf32 as the fused
     multiply-add (one rounding).
The table holds the scores z_s themselves: the identity term fmaf(ident[s], plane value, acc_s) is applied per slot and commutes with
choosing the slot, so the table may be glf_graph_synthesize's planes. Slots the call does not use, and one slot past the last, hold
NaN here, so that a read outside the bank shows in the values.
-> (out float32 [nout, N], lo int [nout, N], hi int [nout, N], f float32 [N]): the indices are returned as well, because a rule that
leaves i uncapped returns the right values (at the top level f = 0 selects z_lo) while its hi leaves the output's bank -- in the kernel
a read past the pixel's row.

`defect` seeds a wrong kernel (tests/test_blend_ref.py shows that the comparison rejects each):
  swap         the lerp weights (and the two selects) exchanged between lo and hi
  uncapped     i = (int)tc, not capped at nlevels - 2: the values survive, hi does not stay in the bank
  no_clamp0    tc = fminf(t, nlevels - 1): a negative level indexes below the bank, a NaN level gives f = NaN
  hi_next      the slot index formed from the uncapped i, f from the capped one: at the top level f = 1 takes hi = the next output's
               level 0
  wrong_half   the image written with acc_row(g, 1 - h): the wrong half-wave owns a slot
  plain_lerp   f * (z_hi - z_lo) + z_lo in place of the pinned form and its f == 1 select (the f == 0 select kept): differs at f = 1 by
               bits
  no_f0        no f == 0 select: the lerp at f = 0 lets an Inf in the unselected slot through as a NaN"""
import numpy as np

from edges_ref import fmaf32

SLOTS = 32
DEFECTS = ("swap", "uncapped", "no_clamp0", "hi_next", "wrong_half", "plain_lerp", "no_f0")


def acc_row(g, h):
    return (g & 3) + 8 * (g >> 2) + 4 * h


def image(table, defect=None):
    """The wave's [SLOTS + 1, N] image of a table [slots <= 32, N]: dealt to the lanes' registers and written back (step 1)."""
    table = np.asarray(table, dtype=np.float32)
    full = np.full((SLOTS, table.shape[1]), np.nan, dtype=np.float32)
    full[:table.shape[0]] = table
    regs = np.empty((2, 16, table.shape[1]), dtype=np.float32)
    for h in range(2):
        for g in range(16):
            regs[h, g] = full[acc_row(g, h)]
    img = np.full((SLOTS + 1, table.shape[1]), np.nan, dtype=np.float32)      # row 32: one past the pixel's row
    for h in range(2):
        for g in range(16):
            img[acc_row(g, 1 - h if defect == "wrong_half" else h)] = regs[h, g]
    return img


def index_rule(level, nlevels, defect=None):
    """(i for the slot index, f float32) of a level map float32 [N] (step 2)."""
    t = np.asarray(level, dtype=np.float32)
    top = np.float32(nlevels - 1)
    with np.errstate(invalid="ignore"):
        tc = np.fmin(t if defect == "no_clamp0" else np.fmax(t, np.float32(0.0)), top)   # fmax / fmin return the operand that is no NaN
        it = np.where(np.isfinite(tc), tc, np.float32(0.0)).astype(np.int64)            # (int)NaN reads 0 on the device; tc is never Inf
        it = np.where(np.isneginf(tc), np.int64(-2 ** 31), it)                          # ... and (int)-inf saturates (no_clamp0 only)
    capped = np.minimum(it, nlevels - 2)
    i_f = it if defect == "uncapped" else capped
    with np.errstate(invalid="ignore"):
        f = (tc - i_f.astype(np.float32)).astype(np.float32)
    return (it if defect in ("uncapped", "hi_next") else capped), f


def emulate(table, level, nout, nlevels, defect=None):
    assert nout >= 1 and nlevels >= 2 and nout * nlevels <= SLOTS
    img = image(table, defect)
    i, f = index_rule(level, nlevels, defect)
    n = img.shape[1]
    px = np.arange(n)
    out = np.empty((nout, n), dtype=np.float32)
    lo_all, hi_all = np.empty((nout, n), dtype=np.int64), np.empty((nout, n), dtype=np.int64)
    for o in range(nout):
        lo = o * nlevels + i
        hi = lo + 1
        lo_all[o], hi_all[o] = lo, hi
        z_lo, z_hi = img[np.clip(lo, 0, SLOTS), px], img[np.clip(hi, 0, SLOTS), px]      # outside the row: the NaN padding
        if defect == "swap":
            z_lo, z_hi = z_hi, z_lo
        with np.errstate(invalid="ignore", over="ignore"):
            if defect == "plain_lerp":
                mix = (f * (z_hi - z_lo).astype(np.float32)).astype(np.float32) + z_lo
            else:
                mix = fmaf32(f, z_hi, fmaf32(-f, z_lo, z_lo))
        mix = np.asarray(mix, dtype=np.float32)
        pick = mix if defect == "plain_lerp" else np.where(f == 1, z_hi, mix)
        out[o] = pick if defect == "no_f0" else np.where(f == 0, z_lo, pick)
    return out, lo_all, hi_all, f


def special_levels(nlevels, n, rng):
    """A level map float32 [n] (n >= 8 nlevels + 16) that holds every integer level, every half, the float32 neighbours below and above
    every integer, negative levels, levels beyond nlevels - 1, -0, NaN, +inf and -inf, and random fractions elsewhere, shuffled."""
    ints = np.arange(nlevels, dtype=np.float32)
    below, above = np.nextafter(ints, np.float32(-np.inf)), np.nextafter(ints, np.float32(np.inf))
    fixed = np.concatenate([ints, ints[:-1] + np.float32(0.5), below, above,
                            np.array([-0.0, -0.25, -3.0, -1e30, nlevels - 0.5, nlevels, nlevels + 7.5, 1e30, np.nan, np.inf, -np.inf],
                                     dtype=np.float32)]).astype(np.float32)
    assert n >= fixed.size
    level = rng.uniform(-0.5, nlevels - 0.5, size=n).astype(np.float32)
    level[:fixed.size] = fixed
    return level[rng.permutation(n)]
