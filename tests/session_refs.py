"""Shared by tests/test_session_cpu.py and tests/test_session_gpu.py: the numpy model of a session call's index metadata and
the cases both files walk."""
import numpy as np

NEW_SYMBOLS = ("cone_model_get_dims", "cone_session_arena_bytes", "cone_session_workspace", "cone_session_index",
               "cone_session_query_layout", "cone_session_localize_workspace", "cone_session_localize")

MAX_Q_L, MAX_V_L, NUM_QUERIES = 20, 90, 5
OUTPUTS = ("tok_off", "tok_len", "tok_idx", "q_ctx_l", "q_vid_off", "batch_pad", "full_w", "n_valid")


def _mixed(nq, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(1, MAX_Q_L + 1, nq)]


# (token lengths, ctx_l, K): nq 1 / 2 / 64; all 1, all 20, mixed; token sums 255 / 256 / 257 (the layout kernel's 256 threads)
LAYOUT_CASES = [
    ([1], 1, 2), ([20], 900, 20), ([7], 333, 9),
    ([1, 1], 46, 3), ([20, 20], 6000, 20), ([3, 17], 91, 4),
    ([1] * 64, 900, 20), ([20] * 64, 900, 20), (_mixed(64, 3), 33000, 20),
    ([20] * 12 + [15], 900, 20), ([20] * 12 + [16], 900, 20), ([20] * 12 + [17], 900, 20),
    (_mixed(17, 5), 45, 2),
]


def layout_model(tok_len, ctx_l, K, num_queries=NUM_QUERIES, max_v_l=MAX_V_L):
    """What one call's metadata must be, from first principles: prefix sums of the lengths, a position counter that restarts
    with every query, and the localizer's constants (every window counts as padded to max_v_l; K * num_queries candidate rows
    per query)."""
    n = np.asarray(tok_len, dtype=np.int64)
    nq = len(n)
    off = np.concatenate([[0], np.cumsum(n)])
    idx = np.concatenate([np.arange(k) for k in n])
    const = lambda v, size: np.full(size, v, dtype=np.int32)
    return dict(tok_off=off.astype(np.int32), tok_len=n.astype(np.int32), tok_idx=idx.astype(np.int32),
                q_ctx_l=const(ctx_l, nq), q_vid_off=const(0, nq), batch_pad=const(max_v_l, nq),
                full_w=const(max_v_l, nq * K), n_valid=const(K * num_queries, nq))
