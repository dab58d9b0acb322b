"""Shared by tests/test_attention_summary_host.py, tests/test_gpu_attention_summary.py and tools/make_attention_summary_golden.py: the
float64 restatement of the attention rollout that include/plipmi.h plipmi_encode_attention_summary defines, written from the
definition (numpy, no GPU), the pooled-row rule, and the error bound the GPU tests hold the rollout kernel to."""
import numpy as np


def rollout_ref(attentions) -> np.ndarray:
    """attentions: L arrays [B, H, S, S] (or one [L, B, H, S, S]) -> float64 [B, S, S]: R_L with R_0 = I and
    R_l = (1/2 mean_h P_l + 1/2 I) R_{l-1} (Abnar & Zuidema 2020, residual weight 1/2, head mean)."""
    first = np.asarray(attentions[0])
    B, _, S, _ = first.shape
    eye = np.eye(S, dtype=np.float64)
    R = np.broadcast_to(eye, (B, S, S)).copy()
    for P in attentions:
        a_hat = 0.5 * np.asarray(P, dtype=np.float64).mean(axis=1) + 0.5 * eye
        R = a_hat @ R
    return R


def pooled_rows(tower: str, B: int, ids=None, eos_token_id: int = -1) -> np.ndarray:
    """r_b: row 0 (CLS) for the vision tower, the row the eos_token_id rule of plipmi_encode_text pools for the text tower"""
    if tower == "vision":
        return np.zeros(B, dtype=np.int64)
    from oracle.clip_oracle import eos_positions
    return np.asarray(eos_positions(np.asarray(ids), eos_token_id), dtype=np.int64)


def rollout_bound(steps: int, S: int, H: int) -> float:
    """Max-abs error of `steps` rollout steps in fp32 against float64 arithmetic on the same fp32 probabilities.  Every quantity of a
    step is a convex combination of values in [0, 1], so each fp32 rounding costs at most 2^-24 absolute: H adds for the head sum,
    the scaling by 1 / (2 H) and its constant, the diagonal add (the "+ 4" covers these with one to spare), and S fused multiply-adds
    for the product.  The factor 1/2 A + 1/2 I is row-(sub)stochastic, so the error R_{l-1} carries is not amplified: errors add
    over the steps."""
    return steps * (S + H + 4) * 2.0 ** -24
