"""The operand maps of the level-0 / level-1 P.V product on the 16x16x32 MFMA shape (csrc/win_frag.h: mfma16_f16, pv_match;
kernels_win24.hip: pv_src24; kernels_win48.hip: pv_src48), restated in numpy and held to O^T = V^T . P^T.

What is modelled: LDS as an array of 16-byte slots (8 f16 each) holding the V^T image blocks exactly as the kernels write them
(block ps, slot 32 hf + vch = the 8 keys of pv-step ps that lane half hf holds in its S^T accumulator) followed by the 4 KB zero
region; the lane's base slot (a matching lane: its image slot, every other lane: 128 bytes into the zeros), the head / pv-step
immediates, the instruction's A / B / D lane maps, and the P fragment as pack8_f16 leaves it.  No GPU."""
import numpy as np
import pytest

ZERO_SLOTS, ZERO_BASE = 4096 // 16, 128 // 16


def rho(i, hf):
    return (i & 3) + 8 * (i >> 2) + 4 * hf


def key_of(ps, hf, j):
    """key (0..63) of element j of pv-step ps in lane half hf: register 8 (ps & 1) + j of the S^T tile of key tile ps >> 1"""
    return 32 * (ps >> 1) + rho(8 * (ps & 1) + j, hf)


def mfma_16x16x32(a, b):
    """a, b: [lane 64][8].  A: lane = row m + 16 kg, B: lane = column n + 16 kg, k = 8 kg + j.  D: [lane][4], register j of lane l =
    row 4 (l >> 4) + j, column l & 15."""
    A = a.reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)      # [m][k]
    B = b.reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)      # [n][k]
    D = A @ B.T
    return np.stack([[D[4 * (l >> 4) + j, l & 15] for j in range(4)] for l in range(64)])


def pv_match(lane):
    return ((lane >> 4) & 1) == ((lane >> 2) & 1)


def p_fragments(P):
    """[ps][lane][j]: the lane's 8 probabilities of pv-step ps (lane = query r + 32 hf)"""
    return np.array([[[P[l & 31, key_of(ps, l >> 5, j)] for j in range(8)] for l in range(64)] for ps in range(4)])


def vt_blocks(V):
    """V: [key 64][vch 32] -> [ps 4][slot 64][8]"""
    return np.array([[[V[key_of(ps, s >> 5, j), s & 31] for j in range(8)] for s in range(64)] for ps in range(4)])


@pytest.mark.parametrize("first_block", [0, 8, 44])      # where the chunk's blocks start: buffer / stream / chunk offsets are part of the base
def test_level0_four_rows_per_head(first_block):
    rng = np.random.default_rng(24)
    P, V = rng.random((32, 64)), rng.standard_normal((64, 32))
    lds = rng.standard_normal((first_block + 4 + 3, 64, 8))        # blocks of other chunks around: garbage that must not be read
    lds[first_block:first_block + 4] = vt_blocks(V)
    zreg = lds.shape[0] * 64
    lds = np.concatenate([lds.reshape(-1, 8), np.zeros((ZERO_SLOTS, 8))])
    pf = p_fragments(P)
    want = P @ V                                                   # [query][vch]
    base = [first_block * 64 + (l & 32) + (l & 3) if pv_match(l) else zreg + ZERO_BASE for l in range(64)]
    for h in range(8):
        t = np.zeros((64, 4))
        for ps in range(4):
            imm = ps * 64 + h * 4                                  # slots: ps * 1024 + h * 64 bytes
            assert all(b + imm < zreg + ZERO_SLOTS for b in base)
            t += mfma_16x16x32(lds[[b + imm for b in base]], pf[ps])
        for l in range(64):                                        # both lane halves receive the head's four rows of the lane's query
            np.testing.assert_allclose(t[l], want[l & 31, 4 * h:4 * h + 4], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("vsteps,chunk", [(4, 0), (16, 0), (16, 3)])   # 8x8 windows; 16x16 windows, first and last chunk
def test_level1_eight_rows_per_head_split_over_the_lane_halves(vsteps, chunk):
    rng = np.random.default_rng(48)
    P, V = rng.random((32, 64)), rng.standard_normal((64, 64))     # 8 heads x 8 rows = two V^T tiles of 32 virtual channels
    lds = rng.standard_normal((2 * vsteps, 64, 8))                 # [tile][pv-step of the window][slot]
    for T in range(2):
        lds[T * vsteps + 4 * chunk:T * vsteps + 4 * chunk + 4] = vt_blocks(V[:, 32 * T:32 * T + 32])
    zreg = lds.shape[0] * 64
    lds = np.concatenate([lds.reshape(-1, 8), np.zeros((ZERO_SLOTS, 8))])
    pf = p_fragments(P)
    want = P @ V
    for h in range(8):
        T, hq = h >> 2, h & 3
        base = [(T * vsteps + 4 * chunk) * 64 + (l & 32) + ((l >> 1) & 4) + (l & 3) if pv_match(l) else zreg + ZERO_BASE for l in range(64)]
        t = np.zeros((64, 4))
        for ps in range(4):
            imm = ps * 64 + hq * 8                                 # ps * 1024 + hq * 128 bytes
            assert all(b + imm < zreg + ZERO_SLOTS for b in base)
            t += mfma_16x16x32(lds[[b + imm for b in base]], pf[ps])
        for l in range(64):                                        # lane half 0: rows 0..3 of the head, lane half 1: rows 4..7
            r0 = 8 * h + 4 * (l >> 5)
            np.testing.assert_allclose(t[l], want[l & 31, r0:r0 + 4], rtol=1e-12, atol=1e-12)


def test_zero_base_keeps_clear_of_the_matching_lanes_banks():
    """Within one 16-lane group of the A read the matching lanes read a 64-byte run at (immediate) mod 256 (level 1: two adjacent runs,
    row groups g >> 1 = 0 and 1) and the others one address: 128 bytes further on, in other banks for every immediate."""
    for imm in range(0, 4 * 1024, 64):
        run = {(imm + 64 * g2 + 16 * c + 4 * d) // 4 % 64 for g2 in range(2) for c in range(4) for d in range(4)}
        zero = {(imm + 16 * ZERO_BASE + 4 * d) // 4 % 64 for d in range(4)}
        assert not run & zero
