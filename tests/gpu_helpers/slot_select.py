"""Shared by tests/test_gpu_slot_select.py and its child process: hbls_slot_select_device on the
bench inputs (bench.setup_inputs: the shares of a validator come from one polynomial, so every
correct aggregate, whatever its member set, equals root_sigs[v]), the corruption recipes of
bench.corrupt applied at chosen items, and the numpy restatement of the selection rule.

As a program: one call under the environment it was started with (HBLS_KEY_LEARN=0, say); prints one
JSON line with the sha256 of every output array."""
import ctypes
import hashlib
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED, COMBINE_FAILED, BAD_INPUT, UNCHECKED = 0, 1, 2, 3, 4, 6, 7
NONE = 0xFFFFFFFF
OTHER_ROOT = hashlib.sha256(b"another signing root").digest()


def _p(x):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    return ctypes.c_void_p(x.data_ptr())


def chk(L, rc):
    assert rc == 0, L.hbls_last_error().decode()


def inputs(L, n, t, V=256):
    import bench
    return bench.setup_inputs(L, dict(n=n, t=t, distinct=False, n_msgs=4), V, 0)


def corrupt_at(L, d, sigs, items):
    """bench.corrupt's five byte recipes at the given items [(partial, class)], in place on sigs
    (NP x 96); returns the expected verification status of every partial."""
    n, NP = d["n"], d["NP"]
    with open(os.path.join(ROOT, "tests", "golden", "off_subgroup_g2.json")) as f:
        offsub = [bytes.fromhex(x) for x in json.load(f)["points"]]
    orig = d["sigs"].reshape(NP, 96)
    exp = np.zeros(NP, dtype=np.uint8)
    rng = random.Random(11)
    wm = [i for i, c in items if c == 2]
    if wm:
        msgs = np.frombuffer(OTHER_ROOT * len(wm), dtype=np.uint8).copy()
        sks = np.concatenate([d["sks"][32 * i:32 * i + 32] for i in wm])
        out, st = np.zeros(96 * len(wm), dtype=np.uint8), np.zeros(len(wm), dtype=np.uint8)
        off, ln = np.arange(len(wm), dtype=np.uint64) * 32, np.full(len(wm), 32, dtype=np.uint32)
        chk(L, L.hbls_sign_batch(_p(sks), _p(msgs), _p(off), _p(ln), len(wm), _p(out), _p(st)))
        assert not st.any()
        sigs[wm] = out.reshape(-1, 96)
    for i, c in items:
        v, sh = divmod(i, n)
        if c == 0:
            b = bytearray(rng.randrange(256) for _ in range(96))
            b[0] &= 0x7F
            sigs[i] = np.frombuffer(bytes(b), dtype=np.uint8)
        elif c == 1:
            sigs[i] = np.frombuffer(offsub[i % len(offsub)], dtype=np.uint8)
        elif c == 3:
            sigs[i] = orig[v * n + (sh + 1) % n]
        elif c == 4:
            sigs[i] = 0
            sigs[i, 0] = 0xC0
        exp[i] = BAD_SIGNATURE if c in (0, 1) else NOT_VERIFIED
    return exp


def all_candidates(d, V=None):
    """Every validator's n partials in share order: (ta_src, ta_idx, grp_off)."""
    n, V = d["n"], d["V"] if V is None else V
    return (np.arange(V * n, dtype=np.uint32), np.tile(np.arange(1, n + 1, dtype=np.int64), V),
            np.arange(V + 1, dtype=np.uint32) * n)


def rule(vst, midx, src, idx, goff, t):
    """The rule of include/hipbls.h restated: (chosen V x t, count V, state V: 0 / UNCHECKED / BAD_INPUT)."""
    V = len(goff) - 1
    chosen, count, state = np.full((V, t), NONE, dtype=np.uint32), np.zeros(V, dtype=np.uint32), np.zeros(V, dtype=np.uint8)
    for g in range(V):
        seen, k = set(), 0
        cand = range(int(goff[g]), int(goff[g + 1]))
        for j in cand:
            if k < t and vst[src[j]] == OK and int(idx[j]) not in seen:
                seen.add(int(idx[j]))
                chosen[g, k] = src[j]
                k += 1
        count[g] = k
        if len({int(midx[src[j]]) for j in cand}) > 1:
            state[g] = BAD_INPUT
        elif k < t:
            state[g] = UNCHECKED
    return chosen, count, state


def run(L, d, t=None, sigs=None, cand=None, vgrp="validator", pks=None, midx=None, V=None, select=True, calls=1):
    """hbls_slot_select_device (select=False: hbls_slot_device with cand as the fixed members) over
    the first V validators of d.  vgrp: "validator" (one verification group each), None (every partial
    its own) or the offsets.  -> dict of host arrays (of the last of `calls` back-to-back calls)."""
    import torch

    from charon_amd import _lib
    dev = torch.device("cuda", 0)
    n, M = d["n"], d["M"]
    V = d["V"] if V is None else V
    t = d["t"] if t is None else t
    NP = V * n
    src, idx, goff = cand if cand is not None else all_candidates(d, V)
    G = len(goff) - 1
    if isinstance(vgrp, str):
        vgrp = np.arange(V + 1, dtype=np.uint32) * n

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    g = dict(msgs=up(d["msgs"]), moff=up(d["moff"].view(np.int64)), mlen=up(d["mlen"].view(np.int32)),
             pks=up((d["pks"] if pks is None else pks)[:NP * 48]),
             sigs=up((d["sigs"] if sigs is None else sigs).reshape(-1)[:NP * 96]),
             midx=up((d["midx"] if midx is None else midx)[:NP].view(np.int32)),
             src=up(np.asarray(src, dtype=np.uint32).view(np.int32) if len(src) else np.zeros(1, np.int32)),
             idx=up(np.asarray(idx, dtype=np.int64) if len(idx) else np.zeros(1, np.int64)),
             goff=up(np.asarray(goff, dtype=np.uint32).view(np.int32)), dvpk=up(d["dv_pks"][:G * 48]))
    if vgrp is not None:
        g["vgoff"] = up(np.asarray(vgrp, dtype=np.uint32).view(np.int32))
    res = None
    s = torch.cuda.Stream(device=dev)
    for _ in range(calls):
        hm = torch.zeros(M * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=dev)
        vst = torch.full((NP,), 255, dtype=torch.uint8, device=dev)
        tout = torch.full((G * 96,), 0x5A, dtype=torch.uint8, device=dev)
        tst = torch.full((G,), 255, dtype=torch.uint8, device=dev)
        ast = torch.full((G,), 255, dtype=torch.uint8, device=dev)
        chosen = torch.full((G * t,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        count = torch.full((G,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        slot = _lib.HblsSlot(msgs=_p(g["msgs"]).value, msg_off=_p(g["moff"]).value, msg_len=_p(g["mlen"]).value,
                             n_msgs=M, hm=_p(hm).value, pks=_p(g["pks"]).value, sigs=_p(g["sigs"]).value,
                             msg_idx=_p(g["midx"]).value, n=NP, vgrp_off=_p(g["vgoff"]).value if vgrp is not None else None,
                             n_vgroups=len(vgrp) - 1 if vgrp is not None else NP, vstatus=_p(vst).value, ta_sigs=None,
                             ta_src=_p(g["src"]).value, ta_idx=_p(g["idx"]).value, grp_off=_p(g["goff"]).value,
                             n_groups=G, n_ta_partials=len(src), ta_out=_p(tout).value, ta_status=_p(tst).value,
                             dv_pks=_p(g["dvpk"]).value, agg_vstatus=_p(ast).value)
        torch.cuda.synchronize()
        if select:
            chk(L, L.hbls_slot_select_device(ctypes.byref(slot), t, _p(chosen), _p(count), ctypes.c_void_p(s.cuda_stream)))
        else:
            chk(L, L.hbls_slot_device(ctypes.byref(slot), ctypes.c_void_p(s.cuda_stream)))
        s.synchronize()
        res = dict(vst=vst.cpu().numpy(), tst=tst.cpu().numpy(), ast=ast.cpu().numpy(),
                   out=tout.cpu().numpy().reshape(G, 96), chosen=chosen.cpu().numpy().view(np.uint32).reshape(G, t),
                   count=count.cpu().numpy().view(np.uint32))
    return res


def skip_case(L, d):
    """Validator v gets candidate position v % 4 corrupted when v % 4 < 3, the corruption cycling
    through the five classes.  -> (sigs NP x 96, expected vstatus)"""
    n, V, NP = d["n"], d["V"], d["NP"]
    sigs = d["sigs"].reshape(NP, 96).copy()
    items = [(v * n + v % 4, k % 5) for k, v in enumerate(v for v in range(V) if v % 4 < 3)]
    return sigs, corrupt_at(L, d, sigs, items)


def digest(res):
    return {k: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for k, a in sorted(res.items())}


def main():
    import torch  # noqa: F401  (the HIP runtime first: charon_amd/_lib.py)

    from charon_amd import _lib
    L = _lib.lib()
    d = inputs(L, 7, 5)
    sigs, _ = skip_case(L, d)
    out = digest(run(L, d, sigs=sigs))
    out["env"] = {k: v for k, v in os.environ.items() if k.startswith("HBLS_")}
    out["key_learn"] = _lib.key_learn_stats(L)[0]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
