"""NumPy restatement of the hard-example selection of average_endpoint_error_hfem (utils.py:268-282): the k pixels that
come first in a stable descending sort of the endpoint-error map -- among equal values the lower flat index first, as
tf.nn.top_k orders them.  Shares no code with src/."""
import numpy as np


def stable_topk_mask(epe, k):
    """Boolean mask (shape of `epe`) of the k entries selected by argsort(-epe, kind="stable")[:k].  NaN counts as the
    largest value (NumPy's argsort would put it last): NaN entries come first, in index order."""
    flat = np.asarray(epe).reshape(-1)
    nan = np.isnan(flat)
    rest = np.nonzero(~nan)[0]
    order = np.concatenate([np.nonzero(nan)[0], rest[np.argsort(-flat[rest], kind="stable")]])
    mask = np.zeros(flat.size, bool)
    mask[order[:int(k)]] = True
    return mask.reshape(np.shape(epe))


def hard_weight(numel, k, lambda_w):
    """(1 + lambda) * #pixels / #hard pixels in fp32 (utils.py:305-312)."""
    return np.float32((1.0 + lambda_w) * (numel / k)) if k > 0 else np.float32(0.0)


def oracle_hard_k(numel, perc):
    """tf.round(perc / 100 * #pixels) in fp32, half to even (utils.py:268-275)."""
    return int(np.round(np.float32(perc / 100) * np.float32(numel)))
