"""The plan of one verification (charon_amd/csrc/vplan.h) on the CPU: which path a call takes and
the sizes that follow, from its shape, the device and the knobs.

* A table of expected fields, written out by hand from the expressions verify_pipeline held before
  they moved into the header: the shapes of tests/test_gpu_launch_trace.py's cases, and the
  per-GPU shapes of BASELINE.json's C2, C3 and C5 at the default knobs on 256 compute units.
* The implications between the fields over seeded random inputs, and the two refusals exactly on
  their conditions.
"""
import ctypes
import random

import pytest

FIELDS = ("n_groups", "gcap", "fbcap", "bfe", "item_always", "first_only", "mmlk", "nb1", "nb2", "nbcap", "smsm",
          "skip_msm", "try_msm", "sides1", "rlc_cmax", "rlc_chunked", "keys_only", "sparse", "lines_at_p", "adaptive")
PROD_FAN = 8
# the library's defaults: HBLS_GROUP_CHUNK, HBLS_FALLBACK_CHUNK, HBLS_FE_BATCH, HBLS_SLOT_MSM, HBLS_RLC_LANES, HBLS_ADAPTIVE
DEFAULT = dict(gcap=131072, fbcap=65536, fe_min=128, smin=32768, lanes=65536, adaptive=1)
NO_FIRST_ERROR = "verify: the first-error mode takes no folded aggregates"
NO_DEFER = "verify: deferred Miller lines need the batched final exponentiation"


@pytest.fixture(scope="module")
def hc():
    from gpu_helpers import harness
    lib = harness.load("hostcheck")
    lib.hc_verify_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.hc_verify_plan.restype = ctypes.c_int
    return lib


def plan(hc, n, n_groups, n_agg=0, grouped=1, first_error=0, defer_msgs=0, n_cu=256, attack=0, **knobs):
    """The plan's fields as a dict, or the refusal's text."""
    k = dict(DEFAULT, **knobs)
    vin = (ctypes.c_uint64 * 14)(n, n_groups, n_agg, grouped, first_error, defer_msgs, n_cu, attack, k["gcap"], k["fbcap"],
                                 k["fe_min"], k["smin"], k["lanes"], k["adaptive"])
    out = (ctypes.c_uint64 * len(FIELDS))()
    err = ctypes.create_string_buffer(128)
    if hc.hc_verify_plan(vin, out, err, len(err)):
        return err.value.decode()
    return dict(zip(FIELDS, (int(v) for v in out)))


def row(n_groups, gcap, fbcap, bfe, item_always, first_only, mmlk, nb1, nb2, nbcap, smsm, skip_msm, sides1, rlc_cmax,
        keys_only, sparse, lines_at_p):
    return dict(n_groups=n_groups, gcap=gcap, fbcap=fbcap, bfe=bfe, item_always=item_always, first_only=first_only,
                mmlk=mmlk, nb1=nb1, nb2=nb2, nbcap=nbcap, smsm=smsm, skip_msm=skip_msm, sides1=sides1,
                rlc_cmax=rlc_cmax, keys_only=keys_only, sparse=sparse, lines_at_p=lines_at_p)


BATCHED = dict(fe_min=128, smin=0)
SLOT_WIDE = dict(fe_min=128, smin=1, adaptive=0)
SLOT = dict(fe_min=128, smin=1)
# (name, the call, the expected fields): by hand, from
#   gcap = min(max(1, GROUP_CHUNK), max(n_groups, 1)); fbcap = min(max(1, FALLBACK_CHUNK), max(n + n_agg, 1))
#   bfe = FE_BATCH && n_groups >= FE_BATCH; item_always = bfe || n_agg; first_only = first_error && bfe
#   mmlk = min(16, max(1, ceil(min(gcap, n_groups) / (21 * 4 * n_cu)))); nb1 = ceil(gcap / mmlk); nb2 = ceil(nb1 / 8)
#   nbcap = max((gcap + 1) / 2, nb1); smsm = bfe && SLOT_MSM && n_groups <= gcap && n + n_agg >= SLOT_MSM
#   skip_msm = smsm && ADAPTIVE && attack; sides1 = smsm && !skip_msm ? 1 : 3
#   rlc_cmax = min(16, max(1, n / RLC_LANES)); keys_only = sides1 == 1 && !(grouped && rlc_cmax > 1)
#   sparse = !(smsm && !skip_msm); lines_at_p = defer_msgs && smsm && !skip_msm
TABLE = [
    ("small_groups", dict(n=5, n_groups=3, fe_min=0), row(3, 3, 5, 0, 0, 0, 1, 3, 1, 3, 0, 0, 3, 1, 0, 1, 0)),
    ("small_ungrouped", dict(n=3, n_groups=0, grouped=0, fe_min=0), row(3, 3, 3, 0, 0, 0, 1, 3, 1, 3, 0, 0, 3, 1, 0, 1, 0)),
    ("per_batch", dict(n=259, n_groups=130, **BATCHED), row(130, 130, 259, 1, 1, 0, 1, 130, 17, 130, 0, 0, 3, 1, 0, 1, 0)),
    ("per_batch_two_chunks", dict(n=259, n_groups=130, gcap=100, **BATCHED),
     row(130, 100, 259, 1, 1, 0, 1, 100, 13, 100, 0, 0, 3, 1, 0, 1, 0)),
    ("slot_wide_per_item", dict(n=259, n_groups=130, **SLOT_WIDE),
     row(130, 130, 259, 1, 1, 0, 1, 130, 17, 130, 1, 0, 1, 1, 1, 0, 0)),
    ("slot_wide_chunked", dict(n=259, n_groups=130, lanes=64, **SLOT_WIDE),
     row(130, 130, 259, 1, 1, 0, 1, 130, 17, 130, 1, 0, 1, 4, 0, 0, 0)),
    ("slot_wide_two_chunks", dict(n=259, n_groups=130, gcap=100, **SLOT_WIDE),
     row(130, 100, 259, 1, 1, 0, 1, 100, 13, 100, 0, 0, 3, 1, 0, 1, 0)),
    ("adaptive_tried", dict(n=259, n_groups=130, **SLOT), row(130, 130, 259, 1, 1, 0, 1, 130, 17, 130, 1, 0, 1, 1, 1, 0, 0)),
    ("adaptive_skipped", dict(n=259, n_groups=130, attack=1, **SLOT),
     row(130, 130, 259, 1, 1, 0, 1, 130, 17, 130, 1, 1, 3, 1, 0, 1, 0)),
    ("attack_without_adaptive", dict(n=259, n_groups=130, attack=1, **SLOT_WIDE),
     row(130, 130, 259, 1, 1, 0, 1, 130, 17, 130, 1, 0, 1, 1, 1, 0, 0)),
    ("first_error_batched", dict(n=259, n_groups=130, first_error=1, **BATCHED),
     row(130, 130, 259, 1, 1, 1, 1, 130, 17, 130, 0, 0, 3, 1, 0, 1, 0)),
    ("first_error_small", dict(n=5, n_groups=3, first_error=1, **BATCHED), row(3, 3, 5, 0, 0, 0, 1, 3, 1, 3, 0, 0, 3, 1, 0, 1, 0)),
    ("slot_dv", dict(n=390, n_groups=130, n_agg=130, **SLOT), row(130, 130, 520, 1, 1, 0, 1, 130, 17, 130, 1, 0, 1, 1, 1, 0, 0)),
    ("slot_no_dv", dict(n=390, n_groups=130, **SLOT), row(130, 130, 390, 1, 1, 0, 1, 130, 17, 130, 1, 0, 1, 1, 1, 0, 0)),
    ("slot_deferred_slot_wide", dict(n=390, n_groups=130, n_agg=130, defer_msgs=130, **SLOT),
     row(130, 130, 520, 1, 1, 0, 1, 130, 17, 130, 1, 0, 1, 1, 1, 0, 1)),
    ("slot_deferred_per_batch", dict(n=390, n_groups=130, n_agg=130, defer_msgs=130, **BATCHED),
     row(130, 130, 520, 1, 1, 0, 1, 130, 17, 130, 0, 0, 3, 1, 0, 1, 0)),
    ("small_with_aggregates", dict(n=12, n_groups=3, n_agg=3), row(3, 3, 15, 0, 1, 0, 1, 3, 1, 3, 0, 0, 3, 1, 0, 1, 0)),
    # BASELINE.json per GPU, default knobs, 256 compute units (one round of waves: 21504 groups)
    ("C2", dict(n=40_000, n_groups=10_000, n_agg=10_000),
     row(10_000, 10_000, 50_000, 1, 1, 0, 1, 10_000, 1250, 10_000, 1, 0, 1, 1, 1, 0, 0)),
    ("C3", dict(n=1_000_000, n_groups=100_000, n_agg=100_000, defer_msgs=100_000),
     row(100_000, 100_000, 65_536, 1, 1, 0, 5, 20_000, 2500, 50_000, 1, 0, 1, 15, 0, 0, 1)),
    ("C5_first_slot", dict(n=875_000, n_groups=125_000, n_agg=125_000),
     row(125_000, 125_000, 65_536, 1, 1, 0, 6, 20_834, 2605, 62_500, 1, 0, 1, 13, 0, 0, 0)),
    ("C5_under_attack", dict(n=875_000, n_groups=125_000, n_agg=125_000, attack=1),
     row(125_000, 125_000, 65_536, 1, 1, 0, 6, 20_834, 2605, 62_500, 1, 1, 3, 13, 0, 1, 0)),
]


@pytest.mark.parametrize("name,call,want", TABLE, ids=[t[0] for t in TABLE])
def test_plan_table(hc, name, call, want):
    got = plan(hc, **call)
    assert isinstance(got, dict), got
    assert {k: got[k] for k in want} == want


def test_implications_and_refusals(hc):
    rng = random.Random(20261020)
    seen = {"smsm": 0, "skip": 0, "first_only": 0, "lines_at_p": 0, NO_FIRST_ERROR: 0, NO_DEFER: 0}
    for _ in range(4000):
        n = rng.choice((1, 2, 5, 100, 259, 4000, 70_000, 1_000_000))
        grouped = rng.random() < 0.8
        n_groups = rng.randint(1, n) if grouped else rng.choice((0, 7))
        groups = n_groups if grouped else n
        n_agg = rng.choice((0, 0, groups))
        first_error = rng.random() < 0.25
        knobs = dict(gcap=rng.choice((0, 1, 100, 5000, 131072)), fbcap=rng.choice((1, 97, 65536)),
                     fe_min=rng.choice((0, 1, 4, 128, 100_000)), smin=rng.choice((0, 1, 64, 32768)),
                     lanes=rng.choice((1, 64, 65536)), adaptive=rng.randint(0, 1))
        defer_msgs = rng.choice((0, 0, groups))
        call = dict(n=n, n_groups=n_groups, n_agg=n_agg, grouped=int(grouped), first_error=int(first_error),
                    defer_msgs=defer_msgs, n_cu=rng.choice((1, 64, 256, 304)), attack=rng.randint(0, 1), **knobs)
        p = plan(hc, **call)
        bfe = bool(knobs["fe_min"]) and groups >= knobs["fe_min"]
        # the two refusals, exactly on their conditions (the first-error one first)
        if first_error and n_agg:
            assert p == NO_FIRST_ERROR, call
        elif defer_msgs and not bfe:
            assert p == NO_DEFER, call
        else:
            assert isinstance(p, dict), (p, call)
        if not isinstance(p, dict):
            seen[p] += 1
            continue
        assert p["n_groups"] == groups and p["bfe"] == bfe, call
        if p["smsm"]:
            assert p["bfe"] and p["n_groups"] <= p["gcap"], call
        if p["skip_msm"]:
            assert p["smsm"] and knobs["adaptive"] and call["attack"], call
        assert p["try_msm"] == (p["smsm"] and not p["skip_msm"]), call
        if p["lines_at_p"]:
            assert p["smsm"] and not p["skip_msm"], call
        if p["first_only"]:
            assert p["bfe"] and not n_agg, call
        assert (p["sides1"] == 1) == bool(p["smsm"] and not p["skip_msm"]) and p["sides1"] in (1, 3), call
        assert p["nb2"] == -(-p["nb1"] // PROD_FAN), call
        assert 1 <= p["mmlk"] <= 16, call
        assert 1 <= p["gcap"] <= max(groups, 1) and 1 <= p["fbcap"] <= max(n + n_agg, 1), call
        assert p["sparse"] == (not p["try_msm"]) and p["adaptive"] == knobs["adaptive"], call
        if p["keys_only"]:
            assert p["sides1"] == 1 and not p["rlc_chunked"], call
        seen["smsm"] += p["smsm"]
        seen["skip"] += p["skip_msm"]
        seen["first_only"] += p["first_only"]
        seen["lines_at_p"] += p["lines_at_p"]
    assert all(v >= 20 for v in seen.values()), seen  # every branch was drawn
