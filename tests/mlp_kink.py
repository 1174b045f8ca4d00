"""The leaky ReLU's kink in a comparison of the MLP head's backward with float64 (shared by tests/test_gpu_ops.py and
tests/test_gpu_mlp_forms.py).

Of the n x hidden pre-activations a handful lie within fp32 rounding of zero; whether such a unit takes slope 1 or alpha - or
0, when the fp32 sum is exactly zero - is decided by the last bit of an fp32 sum, and ONE unit on another branch moves its row
of dx, its column of dW1 and its entry of db1 by (1 - alpha) g_ik.  Every unit whose float64 pre-activation is within
THRESHOLD of zero is AMBIGUOUS; for each one the reference is moved to the branch the kernel took (read off db1, which the
unit touches in one entry, and off the unit's row of dx).  After that a kernel must match float64 like anywhere else."""
import itertools

import torch

THRESHOLD = 1e-6


def ambiguous_units(h, skip_exact_zeros=False):
    """[[row, column]] of the float64 pre-activations h within THRESHOLD of zero.  skip_exact_zeros: a pre-activation that is
    exactly zero in every precision (a zero row of x on a zero bias) is no rounding matter: its slope is 0, and is checked."""
    near = h.abs() < THRESHOLD
    if skip_exact_zeros:
        near &= h != 0
    return near.nonzero().tolist()


def resolve(ref, got, amb, g, slope, xd, W1d, alpha=0.1, max_units=399, max_per_col=6):
    """Moves ref["db1"], ref["dW1"] and ref["dx"] (float64, in place) to the slopes `got` took at the ambiguous units `amb`.
    g = dy W2^T (d loss / d lrelu(h)), slope = the reference's lrelu'(h), xd / W1d the float64 inputs.  Returns the number of
    units moved in (dW1 / db1, dx): the backward may be two launches that each recompute the hidden layer."""
    assert len(amb) <= max_units, "ambiguous units must be few"

    def moves(i, k):
        """what dh[i, k] changes by if the unit takes one of the two slopes the reference did not: the other side of the kink,
        or 0 - the gradient of relu(x) - alpha relu(-x) at a pre-activation that is EXACTLY zero in fp32 (model.py:828-830)"""
        s0 = slope[i, k].item()
        return [0.0] + [g[i, k].item() * (s1 - s0) for s1 in (1.0, alpha, 0.0) if s1 != s0]

    by_col = {}
    for i, k in amb:
        by_col.setdefault(k, []).append(i)
    moved = 0
    for k, rows in by_col.items():
        assert len(rows) <= max_per_col
        res = got["db1"][k].item() - ref["db1"][k].item()
        # the choice per ambiguous unit of the column that explains the residual of db1[k] best (usually one unit, in or out)
        best = min(itertools.product(*[moves(i, k) for i in rows]), key=lambda c: abs(res - sum(c)))
        for i, delta in zip(rows, best):
            if delta != 0.0:
                moved += 1
                ref["db1"][k] += delta
                ref["dW1"][:, k] += delta * xd[i]
    # dx comes from a kernel of its own where the backward is two launches (32 input channels: mlp_bwd_dx_split_kernel and
    # mlp_bwd_w_split_kernel each recompute the hidden layer, in different summation orders): its decision per unit is read
    # off the unit's row of dx - the component of the row's residual along W1[:, k]
    moved_dx = 0
    for i, k in amb:
        w = W1d[:, k]
        c = ((got["dx"][i] - ref["dx"][i]) @ w).item() / (w @ w).item()
        delta = min(moves(i, k), key=lambda d: abs(c - d))
        if delta != 0.0:
            moved_dx += 1
            ref["dx"][i] += delta * w
    return moved, moved_dx
