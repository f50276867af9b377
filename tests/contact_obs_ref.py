"""The car-contact observation on the host, bit for bit (csrc/k_contactobs.h holds the definition; csrc/k_carcontacts.h the record layout):
decode an env's raw car<->car manifold store (mcr_debug_read_contacts) and apply the chain of f64 adds and the mask bits.  numpy only."""
import numpy as np

CC_MAX = 24                      # records kept per env (csrc/mcr_kernels.h: MCR_CC_MAX)
CC_WORDS = 20                    # u32 words per record (MCR_CC_WORDS)
STORE_WORDS = CC_MAX * CC_WORDS + 4    # per env: count, overflow mark, joint order (2 words), the records
HULL_BIT, WHEEL_BIT = 1 << 8, 1 << 9


def make_key(car_a, fix_a, car_b, fix_b):
    return car_a | fix_a << 4 | car_b << 8 | fix_b << 12


def decode(store):
    """one env's store [STORE_WORDS] u32 -> its records in store order: (carA, fixA, carB, fixB, [nImp of point 0 .. n-1] as np.float32).
    Nothing behind record count - 1 is looked at."""
    store = np.asarray(store, np.uint32)
    out = []
    for i in range(min(int(store[0]), CC_MAX)):
        rec = store[4 + i * CC_WORDS: 4 + (i + 1) * CC_WORDS]
        key, n = int(rec[0]), min(int(rec[1]) >> 8, 2)
        imps = [rec[8 + 5 * q: 9 + 5 * q].view(np.float32)[0] for q in range(n)]
        out.append((key & 15, (key >> 4) & 15, (key >> 8) & 15, (key >> 12) & 15, imps))
    return out


def contact_obs(stores, N, prev=None, live=None):
    """stores [B, STORE_WORDS] u32 -> (mask [B, N] int32, impulse [B, N, N] float64).
    prev = (mask, impulse): an ACCUMULATING pass — every sum continues from prev's value, the masks are OR-ed, cells no record names keep
    their bits; None: from zero.  live [B] bool (None: all): an env that is not live contributes nothing — zeros, or prev's rows."""
    stores = np.asarray(stores, np.uint32).reshape(-1, STORE_WORDS)
    B = len(stores)
    if prev is None:
        mask, imp = np.zeros((B, N), np.int32), np.zeros((B, N, N), np.float64)
    else:
        mask, imp = np.array(prev[0], np.int32).reshape(B, N).copy(), np.array(prev[1], np.float64).reshape(B, N, N).copy()
    with np.errstate(all="ignore"):
        for e in range(B):
            if live is not None and not live[e]:
                continue
            for ca, fa, cb, fb, imps in decode(stores[e]):
                for a, j, own in ((ca, cb, fa), (cb, ca, fb)):
                    if a >= N or j >= N:
                        continue
                    mask[e, a] |= (1 << j) | (HULL_BIT if own < 4 else WHEEL_BIT)
                    for x in imps:
                        imp[e, a, j] = imp[e, a, j] + np.float64(x)         # one f64 add per point, in store order
    return mask, imp


def accumulate_steps(rows):
    """a macro-step on the host: rows = per env step (stores [B, W], N, live [B] or None) in step order — sub-step 0 from zero, the others
    accumulating (the chain of adds frame_skip's kernel launches form)"""
    prev = None
    for stores, N, live in rows:
        prev = contact_obs(stores, N, prev=prev, live=live)
    return prev


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()
