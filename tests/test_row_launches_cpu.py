"""The checks of test_row_launches_gpu.py bite, shown on every machine: with the CPU emulation of a launch (the fp64 formula, rounded to bf16 where the kernel
rounds) standing in for the kernel's output, ONE row of the last ragged tile 5 % wrong still passes the whole-tensor bound and fails the per-row one; the untouched
emulation passes both.  This is the failure class — a ragged tile, a tile that straddles two trajectories — the per-row checks exist for."""
from tests.test_row_launches_gpu import BF, GLOBAL, LOCAL, MLP_ROUNDS_MS, chain_formula, chain_operands, errors, mlp_formula, mlp_group


def verdicts(kind, out, ref, row=None):
    eg, el = errors(out, ref, row)
    return eg < GLOBAL[kind], el < LOCAL[kind]


def test_one_wrong_row_of_the_mlp_block_passes_globally_and_fails_locally():
    M = MLP_ROUNDS_MS[2]   # 2753 rows: the last tile holds one row
    g = mlp_group(128, 1024, M, "adaln_add", "adaln", 7200, device="cpu")
    ref, emu = mlp_formula(g), mlp_formula(g, BF)
    for kind in ("blk.Y32", "blk.Yact"):
        assert verdicts(kind, emu[kind], ref[kind]) == (True, True), kind
        bad = emu[kind].clone()
        bad[M - 1] *= 1.05
        assert verdicts(kind, bad, ref[kind]) == (True, False), kind


def test_one_wrong_row_of_the_row_chain_passes_globally_and_fails_locally():
    g = chain_operands(128, 256, 16, 2, 17, 3, "B", device="cpu")   # 34 rows: 16-row tiles 1 and 2 straddle the trajectories, the last holds two rows
    ref, emu = chain_formula(g), chain_formula(g, BF)
    for kind, key in (("chain.Q", "Q0"), ("chain.K", "K1"), ("chain.V", "V0")):   # [B, H, T, hd], a row per head; 0.05 / sqrt(34) lies below their 1.2e-2
        assert verdicts(kind, emu[key], ref[key], 16) == (True, True), kind
        bad = emu[key].clone()
        bad[1, :, 16] *= 1.05      # row 33 = (trajectory 1, step 16), every head of it
        assert verdicts(kind, bad, ref[key], 16) == (True, False), kind
