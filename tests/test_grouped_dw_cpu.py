"""plan_grouped_dw (net.py): the layers of a mesh whose weight-gradient GEMM waits for the grouped launch - the sets that
DESIGN.md section 0 states, decided without a GPU."""
from facet_graph_convolution_amd.net import TRUNK, plan_grouped_dw, r_ld

ALL = {lay.name for lay in TRUNK}
MAX_R = 40 << 20        # FGC_GROUPED_DW_MAX_R_MB's default
N0_100K = 122224        # bench.py's default mesh, the 250 x 200 torus
N0_25K = 30848          # the 125 x 100 torus, as bound


def _plan(n0, dtype="f32", mode="auto", windowed=False, training=True, max_r=MAX_R):
    return plan_grouped_dw([n0, n0 // 4, n0 // 16], dtype, True, mode, max_r, windowed, training)


def test_fp32_groups_the_layers_whose_r_is_small():
    assert set(_plan(N0_100K)) == {"conv1", "conv3", "dconv3", "upconv2", "upconv1"}
    assert set(_plan(N0_25K)) == ALL
    # in forward order, the first layer (which has no r of its own) first
    assert _plan(N0_100K) == ("conv1", "conv3", "dconv3", "upconv2", "upconv1")


def test_the_threshold_is_exact_near_40_mb():
    # dconv1 at 25k facets and upconv1's coarse rows (the pair form) at 100k lie just under it
    dconv1 = N0_25K * r_ld(32, True, False) * 4
    upconv1 = N0_100K * r_ld(32, True, False) // 4 * 4
    assert dconv1 <= MAX_R and upconv1 <= MAX_R
    assert "dconv1" in _plan(N0_25K, max_r=dconv1) and "dconv1" not in _plan(N0_25K, max_r=dconv1 - 1)
    assert "upconv1" in _plan(N0_100K, max_r=upconv1) and "upconv1" not in _plan(N0_100K, max_r=upconv1 - 1)


def test_bf16_groups_every_layer():
    assert set(_plan(N0_100K, "bf16", "1")) == ALL and set(_plan(N0_25K, "bf16", "1")) == ALL


def test_nothing_is_grouped_when_switched_off_or_without_a_backward_pass():
    for n0 in (N0_100K, N0_25K):
        assert _plan(n0, mode="0") == () and _plan(n0, "bf16", "0") == ()
        assert _plan(n0, training=False) == () and _plan(n0, "bf16", "1", training=False) == ()


def test_a_shard_with_the_weight_gradients_in_the_exchange_window_groups_the_first_layer_only():
    for n0 in (N0_100K, N0_25K):
        assert _plan(n0, windowed=True) == ("conv1",) and _plan(n0, "bf16", "1", windowed=True) == ("conv1",)
