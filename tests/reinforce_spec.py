"""The arithmetic of daco_reinforce / daco_reinforce_backward (include/deepaco_hip.h) restated in numpy, operation for
operation: float32 throughout, every sum from +0.0 and sequential (r ascending, then a ascending), a product rounded before it
is added, IEEE divisions by float32(A).  The GPU tests hold the kernels to this bit for bit; tests/test_reinforce_spec.py holds
this to a float64 evaluation and to the train cell's torch expression."""
import numpy as np

F = np.float32


def live_rows(R, lens=None, d=0):
    """[B] int32 live rows, or None when lens is None (every instance: R)"""
    if lens is None:
        return None
    live = lens.astype(np.int64).max(axis=1) - int(d)
    return np.clip(live, 0, R).astype(np.int32)


def forward(obj, log_probs, lens=None, d=0, sign=1):
    """obj [B, A] f32, log_probs [B, R, A] f32, lens [B, A] int32 | None -> (loss [B] f32, adv [B, A] f32, live [B] int32)"""
    obj, lp = np.asarray(obj, dtype=F), np.asarray(log_probs, dtype=F)
    B, R, A = lp.shape
    assert obj.shape == (B, A) and sign in (1, -1)
    live = live_rows(R, lens, d)
    if live is None:
        live = np.full(B, R, dtype=np.int32)
    s = np.zeros((B, A), dtype=F)
    for r in range(R):                                    # r ascending; a row past an instance's live rows is not added at all
        on = (r < live)[:, None]
        s = np.where(on, (s + lp[:, r, :]).astype(F), s)
    total = np.zeros(B, dtype=F)
    for a in range(A):                                    # a ascending
        total = (total + obj[:, a]).astype(F)
    mean = (total / F(A)).astype(F)
    adv = (F(sign) * (obj - mean[:, None]).astype(F)).astype(F)
    acc = np.zeros(B, dtype=F)
    for a in range(A):
        acc = (acc + (adv[:, a] * s[:, a]).astype(F)).astype(F)      # the product is rounded, then added
    return (acc / F(A)).astype(F), adv, live


def backward(g, adv, live, R):
    """g [B] f32, adv [B, A] f32, live [B] int32 -> grad_log_probs [B, R, A] f32: (g adv) / A on the live rows, +0.0 past them"""
    g, adv = np.asarray(g, dtype=F), np.asarray(adv, dtype=F)
    B, A = adv.shape
    row = ((g[:, None] * adv).astype(F) / F(A)).astype(F)
    on = (np.arange(R)[None, :] < np.clip(live, 0, R)[:, None])[:, :, None]
    return np.where(on, row[:, None, :], F(0.0)).astype(F)
