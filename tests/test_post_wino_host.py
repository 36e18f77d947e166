"""The algebra of the post-net's Winograd F(4,5) route (csrc/post_wino.h), without a GPU: the matrices the three transform kernels are compiled with,
read back through the diagnostic library's host-only `l2s_op_post_wino_matrices`, turn 8 point-wise products into the four outputs of a 5-tap filter."""
import numpy as np

from lip2speech_amd import native


def test_matrices_give_the_four_output_correlation():
    AT, G, BT = native.op_post_wino_matrices()
    assert AT.shape == (4, 8) and G.shape == (8, 5) and BT.shape == (8, 8)
    rng = np.random.default_rng(5)
    for _ in range(64):
        d, g = rng.standard_normal(8), rng.standard_normal(5)
        want = np.array([np.dot(g, d[i:i + 5]) for i in range(4)])
        got = AT @ ((G @ g) * (BT @ d))
        assert np.abs(got - want).max() <= 1e-12, (got, want)


def test_activation_side_matrices_are_exact_in_fp32():
    """AT and BT are applied in fp32 by the input / output transforms: every entry must be a float (G is applied in fp64 to the weights, once)."""
    AT, _, BT = native.op_post_wino_matrices()
    assert np.array_equal(AT.astype(np.float32).astype(np.float64), AT) and np.array_equal(BT.astype(np.float32).astype(np.float64), BT)


def test_option_is_a_diagnostic_one():
    assert "post_wino" in native.DIAG_OPTIONS and "l2s_op_post_wino_matrices" in native.DIAG_SYMBOLS
