"""The controller of adaptive discriminator augmentation (vg_ada_update) restated in NumPy: nothing
imported from the package.  The sign statistic is summed in Python ints (exact, no order shows); the three rounded
operations of an adjustment -- the division, the product ``count * rate`` and the sum ``p +- step`` -- are each ONE
``np.float32`` operation, which is what the kernel's no-FMA rule buys: the same bits.

State: the eight words of vg_ada_state as a dict -- p, sign_sum, count, calls, rt, adjustments (words 6 and 7 stay 0)."""
import numpy as np

WORDS = ("p", "sign_sum", "count", "calls", "rt", "adjustments")
F32 = np.float32


def state(p0=0.0):
    return dict(p=F32(p0), sign_sum=0, count=0, calls=0, rt=F32(0.0), adjustments=0)


def signs(d, threshold):
    """sum_b ((d[b] > threshold) - (d[b] < threshold)) over fp32 values: a NaN or a tie adds 0."""
    d, t = np.asarray(d, dtype=F32).reshape(-1), F32(threshold)
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(d > t)) - int(np.count_nonzero(d < t))


def update(st, d, threshold, target, rate, interval):
    """One call of the controller on the vector ``d``: returns the NEW state (``st`` is left as it is)."""
    st = dict(st)
    d = np.asarray(d, dtype=F32).reshape(-1)
    st["sign_sum"] += signs(d, threshold)
    st["count"] += int(d.size)
    st["calls"] += 1
    if st["calls"] >= interval:
        rt = F32(st["sign_sum"]) / F32(st["count"])                  # int32 -> fp32 conversions round to nearest, as the kernel's
        direction = int(rt > F32(target)) - int(rt < F32(target))
        with np.errstate(over="ignore"):
            step = F32(st["count"]) * F32(rate)                       # one rounded product
        p = st["p"]
        if direction:
            p = p + step if direction > 0 else p - step               # one rounded sum (x - y is x + (-y): the same rounding)
        p = F32(0.0) if p < 0 else (F32(1.0) if p > 1 else p)         # (comparisons: a NaN p stays a NaN)
        st.update(p=F32(p), rt=F32(rt), adjustments=st["adjustments"] + 1, sign_sum=0, count=0, calls=0)
    return st


def words(st):
    """The eight words as int32 bit patterns: what the device tensor holds."""
    out = np.zeros(8, dtype=np.int32)
    out[0] = np.array([st["p"]], dtype=F32).view(np.int32)[0]
    out[1], out[2], out[3] = st["sign_sum"], st["count"], st["calls"]
    out[4] = np.array([st["rt"]], dtype=F32).view(np.int32)[0]
    out[5] = st["adjustments"]
    return out


def neighbours(v):
    """(the fp32 below v, v, the fp32 above v)"""
    v = F32(v)
    return float(np.nextafter(v, F32(-np.inf))), float(v), float(np.nextafter(v, F32(np.inf)))
