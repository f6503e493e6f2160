"""Reference of a K-class quantised model for the tests: the single-row integer oracle (oracle/int8_oracle.py), one
call per class."""
import numpy as np

from oracle import int8_oracle as Q


def sliced_reference(qm, frames):
    """(N,K,H,W) float32 logits of a K-class quantised model: Q.forward once per class, with the head's arrays
    (output.w_q, w_zp, bias_q, mult) sliced to that row."""
    k = np.asarray(qm["output.bias_q"]).size
    rows = []
    for c in range(k):
        q1 = dict(qm)
        for f in ("w_q", "w_zp", "bias_q", "mult"):
            q1["output." + f] = np.asarray(qm["output." + f])[c:c + 1]
        rows.append(Q.forward(q1, frames))
    return np.concatenate(rows, axis=1)


def softmax64(z):
    """float64 softmax over axis 1"""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)
