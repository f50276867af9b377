"""CPU: the car-contact observation's C ABI (include/mcr.h: mcr_set_contact_obs and its siblings), VecMultiCarRacing's keyword checks, and
the known-answer tests of its numpy restatement (tests/contact_obs_ref.py) on hand-made manifold stores."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import contact_obs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcr_set_contact_obs", "mcr_contact_obs_now", "mcr_contact_store_words", "mcr_debug_read_contacts", "mcr_debug_contact_obs")
MCR_ERR_ARG = -1
NAN_BITS = 0x7fc0dead                   # an f32 NaN with a payload: must never reach a sum


def _store(records, count=None):
    """one env's store from records (carA, fixA, carB, fixB, [nImp, ..]): every word that is not defined is NaN_BITS"""
    s = np.full(R.STORE_WORDS, NAN_BITS, np.uint32)
    s[0] = len(records) if count is None else count
    s[1:4] = 0
    for i, (ca, fa, cb, fb, imps) in enumerate(records):
        rec = s[4 + i * R.CC_WORDS: 4 + (i + 1) * R.CC_WORDS]
        rec[0] = R.make_key(ca, fa, cb, fb)
        rec[1] = 1 | len(imps) << 8
        for q, x in enumerate(imps):
            rec[8 + 5 * q] = np.array([x], np.float32).view(np.uint32)[0]
    return s


def test_symbols_exported_declared_and_sized(lib):
    L = lib.load()
    src = open(os.path.join(ROOT, "include", "mcr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert re.search(r"\bint\s+%s\s*\(" % n, code), f"{n} is not declared in include/mcr.h"
        assert n in lib.SYMBOLS
    kern = open(os.path.join(ROOT, "multi_car_racing_amd", "csrc", "mcr_kernels.h")).read()
    cc_max = int(re.search(r"#define MCR_CC_MAX (\d+)", kern).group(1)); cc_words = int(re.search(r"#define MCR_CC_WORDS (\d+)", kern).group(1))
    assert lib.contact_store_words() == (cc_max, cc_max * cc_words + 4, cc_words)
    assert (R.CC_MAX, R.STORE_WORDS, R.CC_WORDS) == lib.contact_store_words()
    assert L.mcr_contact_store_words(None, None) == cc_max


def test_argument_checks_without_a_device(lib):
    L = lib.load()
    buf = np.zeros(16, np.float64)
    # exactly one pointer null: refused whatever the handle
    assert L.mcr_set_contact_obs(None, lib.ptr(buf), None) == MCR_ERR_ARG and b"exactly one" in L.mcr_last_error()
    assert L.mcr_set_contact_obs(None, None, lib.ptr(buf)) == MCR_ERR_ARG and b"exactly one" in L.mcr_last_error()
    assert L.mcr_set_contact_obs(None, None, None) == MCR_ERR_ARG and b"null handle" in L.mcr_last_error()
    assert L.mcr_contact_obs_now(None, None) == MCR_ERR_ARG
    assert L.mcr_debug_read_contacts(None, lib.ptr(buf)) == MCR_ERR_ARG
    p = lib.ptr(buf)
    for args in ((None, 1, 2, 0, p, p), (p, 1, 2, 0, None, p), (p, 1, 2, 0, p, None), (p, 0, 2, 0, p, p), (p, 1, 1, 0, p, p), (p, 1, 9, 0, p, p)):
        assert L.mcr_debug_contact_obs(*args, None) == MCR_ERR_ARG


def test_keyword_validation_comes_before_anything_is_created(lib):
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    with pytest.raises(ValueError, match="contact_obs"):
        VecMultiCarRacing(4, 1, contact_obs=True)
    with pytest.raises(ValueError, match="contact_obs"):
        VecMultiCarRacing(4, 2, car_contacts=False, contact_obs=True)


# ------------------------------------------------------------------ the reference's own known answers
def test_ref_symmetry_and_order_of_the_sum():
    big, tiny = np.float32(3.0e38), np.float32(1.0e-30)
    recs = [(0, 0, 1, 2, [big]), (0, 1, 1, 2, [tiny]), (0, 1, 1, 3, [-big]), (1, 0, 2, 5, [np.float32(0.25)])]
    mask, imp = R.contact_obs(_store(recs)[None], 3)
    want = (np.float64(big) + np.float64(tiny)) + np.float64(-big)
    assert want == 0.0 and (np.float64(big) + np.float64(-big)) + np.float64(tiny) != 0.0     # the order shows
    assert R.same_bits(imp[0, 0, 1], want) and R.same_bits(imp[0, 0, 1], imp[0, 1, 0])
    assert imp[0, 1, 2] == 0.25 and imp[0, 2, 1] == 0.25 and imp[0, 0, 2] == 0.0 and imp[0, 2, 0] == 0.0
    assert R.same_bits(imp[0], imp[0].T) and (np.diagonal(imp[0]) == 0.0).all()
    assert mask[0].tolist() == [0b010 | R.HULL_BIT, 0b101 | R.HULL_BIT, 0b010 | R.WHEEL_BIT]


def test_ref_hull_and_wheel_bits():
    # car 0's wheel (fixture 6) against car 1's hull polygon 3; the record's lower fixture comes second (a flipped key)
    mask, imp = R.contact_obs(_store([(1, 3, 0, 6, [np.float32(2.0)])])[None], 2)
    assert mask[0].tolist() == [0b10 | R.WHEEL_BIT, 0b01 | R.HULL_BIT] and imp[0, 0, 1] == 2.0 and imp[0, 1, 0] == 2.0
    # fixture 3 is the last hull polygon, fixture 4 the first wheel; both bits of a car can be set at once
    mask, _ = R.contact_obs(_store([(0, 3, 1, 4, [np.float32(1.0)]), (0, 4, 1, 0, [np.float32(1.0)])])[None], 2)
    assert mask[0].tolist() == [0b10 | R.HULL_BIT | R.WHEEL_BIT, 0b01 | R.HULL_BIT | R.WHEEL_BIT]


def test_ref_ignores_what_lies_behind_the_count():
    recs = [(0, 0, 1, 0, [np.float32(1.5)]), (0, 1, 1, 1, [np.float32(4.0)]), (0, 4, 1, 2, [np.float32(8.0)])]
    mask, imp = R.contact_obs(_store(recs, count=1)[None], 2)
    assert imp[0, 0, 1] == 1.5 and mask[0].tolist() == [0b10 | R.HULL_BIT, 0b01 | R.HULL_BIT]
    mask, imp = R.contact_obs(_store(recs, count=0)[None], 2)
    assert not mask.any() and not imp.any()
    # a count beyond the capacity reads the capacity
    full = [(0, 0, 1, 0, [np.float32(1.0)])] * R.CC_MAX
    _, imp = R.contact_obs(_store(full, count=1000)[None], 2)
    assert imp[0, 0, 1] == float(R.CC_MAX)


def test_ref_two_point_record_and_unused_second_point():
    one = _store([(0, 0, 1, 0, [np.float32(1.0)])])                       # its second point's words are NaN bit patterns
    two = _store([(0, 0, 1, 0, [np.float32(1.0), np.float32(0.5)])])
    assert R.contact_obs(one[None], 2)[1][0, 0, 1] == 1.0 and R.contact_obs(two[None], 2)[1][0, 0, 1] == 1.5
    assert len(R.decode(two)[0][4]) == 2 and len(R.decode(one)[0][4]) == 1


def test_ref_accumulation_is_one_chain_and_dead_envs_keep_their_rows():
    a = _store([(0, 0, 1, 0, [np.float32(3.0e38)])]); b = _store([(0, 0, 1, 0, [np.float32(1.0e-30)])]); c = _store([(0, 5, 1, 0, [np.float32(-3.0e38)])])
    stores = [np.stack([s, s]) for s in (a, b, c)]
    live = [None, np.array([True, False]), None]
    mask, imp = R.accumulate_steps([(s, 2, l) for s, l in zip(stores, live)])
    assert imp[0, 0, 1] == 0.0 and imp[1, 0, 1] == 0.0 and R.same_bits(imp[0], imp[0].T)
    assert mask[0].tolist() == [0b10 | R.HULL_BIT | R.WHEEL_BIT, 0b01 | R.HULL_BIT]
    _, imp2 = R.accumulate_steps([(stores[1], 2, None), (stores[0], 2, None), (stores[2], 2, None)])
    assert imp2[0, 0, 1] == 0.0                                            # (tiny + big) - big
    _, imp3 = R.accumulate_steps([(stores[0], 2, None), (stores[2], 2, None), (stores[1], 2, None)])
    assert imp3[0, 0, 1] == np.float64(np.float32(1.0e-30))               # the step order shows
    # an env that is not live in a pass that does not accumulate: zeros
    mask, imp = R.contact_obs(stores[0], 2, live=np.array([False, True]))
    assert not mask[0].any() and not imp[0].any() and imp[1, 0, 1] == np.float64(np.float32(3.0e38))
