"""Build libhipbls.so (gfx950) in-tree, plus the test-only CPU harness, C client and device block
harness.

    python -m charon_amd.build            # product library + test harnesses
The product library is compiled by hipcc for --offload-arch=gfx950 only.
"""

from __future__ import annotations

import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib", "libhipbls.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SOURCES = ["hipbls.hip", "pipeline.hip", "threshold.hip", "vbatch.hip", "vgroup.hip", "roots.hip", "hash.hip", "msm.hip",
           "hashsplit.hip", "duty.hip", "dutyfirst.hip", "cluster.hip", "lockcheck.hip"]


def build_id(defines=()) -> str:
    """The id embedded in the library: the source hash (charon_amd._lib.source_build_id) plus the
    tuning defines of a variant build."""
    from charon_amd._lib import BUILD_ID_PREFIX, source_build_id
    bid = BUILD_ID_PREFIX + source_build_id(ROOT)
    if defines:
        bid += "+" + ",".join(d.replace(" ", "") for d in defines)
    return bid


def build_library(force: bool = False, verbose: bool = True, defines=(), out: str = LIB) -> str:
    """defines / out: experiment variants (-D defines -> charon_amd/lib/variants/...), used by
    tools/ experiments through HBLS_LIBRARY; the product is the default build.  A library whose
    embedded build id equals the tree's is reused; any other is rebuilt."""
    from charon_amd._lib import embedded_build_id
    LIB = out
    bid = build_id(defines)
    if not force and os.path.exists(LIB) and embedded_build_id(LIB) == bid:
        if verbose:
            print(f"reused {LIB} ({bid}: built from these sources)")
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    t = time.time()
    # the translation units compile in parallel (pipeline.hip is the long one), then link
    objs, procs = [], []
    for src in SOURCES:
        obj = os.path.join(os.path.dirname(LIB), os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        extra = [f'-DHBLS_BUILD_ID="{bid}"'] if src == "hipbls.hip" else []
        procs.append(subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c"] +
                                      ["-D" + d for d in defines] + extra + [os.path.join(CSRC, src), "-o", obj]))
    for p in procs:
        if p.wait(timeout=3000) != 0:
            raise RuntimeError("hipcc failed")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB + ".tmp"] + objs +
                   ["-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    os.replace(LIB + ".tmp", LIB)
    if verbose:
        print(f"compiled {LIB} in {time.time() - t:.1f}s ({bid})")
    return LIB


HOSTCHECK_PREFIX = "hbls-hostcheck:"
HOSTCHECK_FLAGS = ["-O3", "-march=x86-64-v3", "-std=c++17", "-pthread", "-shared", "-fPIC"]


def hostcheck_build_id(defines=(), flags=None, root: str = "") -> str:
    """The id embedded in the CPU harness: sha256 (16 hex digits) over the harness source, every
    header of charon_amd/csrc (it includes the kernels' arithmetic from there), the compiler flags
    and the defines -- what `hc_build_id()` of a harness built from this tree returns."""
    import hashlib
    root = root or ROOT
    csrc = os.path.join(root, "charon_amd", "csrc")
    h = hashlib.sha256()
    files = [os.path.join(root, "tests", "native", "hostcheck.cpp")] + \
        sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h"))
    for f in files:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join((flags or HOSTCHECK_FLAGS) + ["-D" + d for d in defines]).encode())
    return HOSTCHECK_PREFIX + h.hexdigest()[:16]


def embedded_hostcheck_id(path: str) -> str:
    """The harness id inside a built harness file, read from its bytes (no loading)."""
    import re
    with open(path, "rb") as f:
        m = re.search(rb"hbls-hostcheck:[0-9a-f]{16}", f.read())
    return m.group(0).decode() if m else ""


def check_hostcheck(path: str, defines=(), root: str = "") -> str:
    """The harness's id if it was built from the tree's sources (with these defines), else raise:
    a stale harness would time or check code the kernels no longer run."""
    got, want = embedded_hostcheck_id(path), hostcheck_build_id(defines, root=root)
    if got != want:
        raise RuntimeError(f"stale CPU harness {path}: built as {got or '(unstamped)'}, the tree is {want}")
    return got


def build_hostcheck(force: bool = False, verbose: bool = True, defines=(), out: str = "") -> str:
    """defines / out: another build of the harness (e.g. ("HB_HOST_MUL28",): the 28-bit host
    products, tests/test_sanitizers.py).  A harness whose embedded id (hc_build_id) equals this
    tree's is reused; any other -- a header touched, other flags -- is rebuilt."""
    src = os.path.join(ROOT, "tests", "native", "hostcheck.cpp")
    out = out or os.path.join(ROOT, "tests", "native", "libhbls_hostcheck.so")
    bid = hostcheck_build_id(defines)
    if not force and os.path.exists(out) and embedded_hostcheck_id(out) == bid:
        return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + ["-D" + d for d in defines] + [f'-DHC_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


WIDECHECK_PREFIX = "hbls-widecheck:"


def widecheck_build_id(root: str = "") -> str:
    """The id embedded in the ladder-table harness (tests/native/widecheck.cpp, `wc_build_id()`):
    sha256 over its source, every header of charon_amd/csrc and the compiler flags, as
    hostcheck_build_id."""
    import hashlib
    root = root or ROOT
    csrc = os.path.join(root, "charon_amd", "csrc")
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "widecheck.cpp")] + \
            sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")):
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return WIDECHECK_PREFIX + h.hexdigest()[:16]


def build_widecheck(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_widecheck.so (tests/test_key_wide_host.py): the learned keys' ladder
    tables and the ladders through them on the CPU; test-only.  Reused when its embedded id equals
    the tree's, as build_hostcheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "widecheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_widecheck.so")
    bid = widecheck_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-widecheck:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DWC_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


TASELCHECK_PREFIX = "hbls-taselcheck:"


def taselcheck_build_id(root: str = "") -> str:
    """The id embedded in the member-selection harness (tests/native/taselcheck.cpp, `ts_build_id()`):
    sha256 over its source, the one header it compiles (charon_amd/csrc/tasel.h) and the flags."""
    import hashlib
    root = root or ROOT
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "taselcheck.cpp"),
              os.path.join(root, "charon_amd", "csrc", "tasel.h")]:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return TASELCHECK_PREFIX + h.hexdigest()[:16]


def build_taselcheck(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_taselcheck.so (tests/test_tasel_host.py): the verified-member selection
    rule of hbls_slot_select_device on the CPU; test-only.  Reused when its embedded id equals the
    tree's, as build_hostcheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "taselcheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_taselcheck.so")
    bid = taselcheck_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-taselcheck:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DTS_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


SLOTHOSTCHECK_PREFIX = "hbls-slothostcheck:"
SLOTHOSTCHECK_HEADERS = ("hslot.h", "hgroup.h", "msgtable.h", "tasel.h")


def slothostcheck_build_id(root: str = "") -> str:
    """The id embedded in the host-buffer duty's harness (tests/native/slothostcheck.cpp,
    `hs_build_id()`): sha256 over its source, the headers it compiles and the flags."""
    import hashlib
    root = root or ROOT
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "slothostcheck.cpp")] + \
            [os.path.join(root, "charon_amd", "csrc", f) for f in SLOTHOSTCHECK_HEADERS]:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return SLOTHOSTCHECK_PREFIX + h.hexdigest()[:16]


def build_slothostcheck(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_slothostcheck.so (tests/test_hslot.py): the host plan of
    hbls_slot_select_batch and its matching rule on the CPU; test-only.  Reused when its embedded id
    equals the tree's, as build_hostcheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "slothostcheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_slothostcheck.so")
    bid = slothostcheck_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-slothostcheck:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DHS_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


DUTYCHECK_PREFIX = "hbls-dutycheck:"
DUTYCHECK_HEADERS = ("dutysel.h", "hduty.h", "hslot.h", "hgroup.h", "msgtable.h", "tasel.h")


def dutycheck_build_id(root: str = "") -> str:
    """The id embedded in the duty sessions' harness (tests/native/dutycheck.cpp, `dc_build_id()`):
    sha256 over its source, the headers it compiles and the flags."""
    import hashlib
    root = root or ROOT
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "dutycheck.cpp")] + \
            [os.path.join(root, "charon_amd", "csrc", f) for f in DUTYCHECK_HEADERS]:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return DUTYCHECK_PREFIX + h.hexdigest()[:16]


def build_dutycheck(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_dutycheck.so (tests/test_duty_host.py): the storing and firing rule of a
    duty session and the host plan of hbls_duty_add on the CPU; test-only.  Reused when its embedded
    id equals the tree's, as build_hostcheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "dutycheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_dutycheck.so")
    bid = dutycheck_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-dutycheck:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DDC_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


DUTYSETCHECK_PREFIX = "hbls-dutysetcheck:"
DUTYSETCHECK_HEADERS = ("dutysel.h", "hduty.h", "hslot.h", "hgroup.h", "msgtable.h")


def dutysetcheck_build_id(root: str = "") -> str:
    """The id embedded in the set-atomic adds' harness (tests/native/dutysetcheck.cpp,
    `ds_build_id()`): sha256 over its source, the headers it compiles and the flags."""
    import hashlib
    root = root or ROOT
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "dutysetcheck.cpp")] + \
            [os.path.join(root, "charon_amd", "csrc", f) for f in DUTYSETCHECK_HEADERS]:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return DUTYSETCHECK_PREFIX + h.hexdigest()[:16]


def build_dutysetcheck(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_dutysetcheck.so (tests/test_duty_sets_host.py): the host side of
    hbls_duty_add_sets on the CPU -- set_off's validation, the plan's set ids, the shards' merge, the
    admission predicate and the storing rule behind it; test-only.  Reused when its embedded id
    equals the tree's, as build_dutycheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "dutysetcheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_dutysetcheck.so")
    bid = dutysetcheck_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-dutysetcheck:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DDS_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


SUBGCHECK_PREFIX = "hbls-subgcheck:"
SUBGCHECK_HEADERS = ("subgbatch.h", "sha256.h", "hd.h", "vplan.h")


def subgcheck_build_id(root: str = "") -> str:
    """The id embedded in the batched subgroup test's harness (tests/native/subgcheck.cpp,
    `sg_build_id()`): sha256 over its source, the headers it compiles and the flags."""
    import hashlib
    root = root or ROOT
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "subgcheck.cpp")] + \
            [os.path.join(root, "charon_amd", "csrc", f) for f in SUBGCHECK_HEADERS]:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return SUBGCHECK_PREFIX + h.hexdigest()[:16]


def build_subgcheck(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_subgcheck.so (tests/test_subgroup_batch_host.py): the batched subgroup
    test's digits and its plan on the CPU; test-only.  Reused when its embedded id equals the tree's,
    as build_hostcheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "subgcheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_subgcheck.so")
    bid = subgcheck_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-subgcheck:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DSG_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


def build_c_client(force: bool = False, verbose: bool = True) -> str:
    """tests/native/cabi_client: a C program linked against libhipbls.so through include/hipbls.h
    (what the Go shim's cgo does), compiled with -std=c99 -Wall -Wextra -Werror so the header is
    checked as C; test-only."""
    src = os.path.join(ROOT, "tests", "native", "cabi_client.c")
    out = os.path.join(ROOT, "tests", "native", "cabi_client")
    deps = [src, os.path.join(ROOT, "include", "hipbls.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-o", out + ".tmp", src,
           "-L" + os.path.dirname(LIB), "-lhipbls", "-Wl,-rpath," + os.path.dirname(LIB),
           "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, timeout=300)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


DEVBLOCKS_PREFIX = "hbls-devblocks:"
DEVBLOCKS_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# the translation units of one build: (source, its defines, object name); the lane-group file once
# per group kind (Grp, Grp6, Grp18), each well below pipeline.hip's compile time
DEVBLOCKS_UNITS = [("devblocks_leaf.hip", [], "leaf")] + \
    [("devblocks_grp.hip", [f"-DDB_GK={k}"], f"grp{k}") for k in range(3)]
# the two builds: fp.h's default HB_ARG_LANES (64: vbatch.hip, threshold.hip, msm.hip,
# hashsplit.hip) and pipeline.hip's 128
DEVBLOCKS_BUILDS = {"64": [], "128": ["-DHB_ARG_LANES=128"]}
# The curve layer (tests/test_gpu_curve.py) is a harness of its own, libhbls_devblockscurve.so, with
# an id of its own: the curve kernels use fp.h's default HB_ARG_LANES only, and the block harnesses
# above neither change nor rebuild when a curve source does.  Its units: the point operations of G1
# and G2, the ladders, and the bucket MSM, whose unit compiles the product's msm.hip itself
# (DEVBLOCKS_PRODUCT_SOURCES: hashed into the id).
DEVBLOCKS_CURVE = "curve"
DEVBLOCKS_CURVE_UNITS = [("devblocks_curve.hip", [f"-DDB_CV={k}"], f"cv{k}") for k in (1, 2, 3)] + \
    [("devblocks_msm.hip", [], "msm")]
# Hash-to-curve (tests/test_gpu_hash.py) is a third harness, libhbls_devblockshash.so, on the same
# terms: the fast-convention unit in two parts (1: the stages, compiling the product's hashsplit.hip
# itself; 2: the leaves) and the standard-convention unit (as hash.hip is compiled).
DEVBLOCKS_HASH = "hash"
DEVBLOCKS_HASH_UNITS = [("devblocks_h2c.hip", [f"-DDB_H2C={k}"], f"h2c{k}") for k in (1, 2)] + \
    [("devblocks_h2c_std.hip", [], "h2cstd")]
# The Miller-loop kernels and the group stage (tests/test_gpu_pairing.py) are a fourth harness,
# libhbls_devblockspair.so: one unit compiles the product's pipeline.hip itself (which sets its own
# HB_FAST_FPMUL and HB_ARG_LANES 128: the build passes neither), the other vgroup.hip with fp.h's
# default lanes, as the library compiles the two.  The pipeline unit is not split: it includes
# pipeline.hip whole, so its compile time is that file's own.
DEVBLOCKS_PAIR = "pair"
DEVBLOCKS_PAIR_UNITS = [("devblocks_pair.hip", [], "pair"), ("devblocks_vgroup.hip", [], "vgroup")]
# The combination and verdict kernels of the batched verification (tests/test_gpu_vbatch.py) are a
# fifth harness, libhbls_devblocksvb.so: one unit, which compiles the product's vbatch.hip itself
# (fp.h's default lanes; vbatch.hip sets its own HB_FAST_FPMUL).  Not split: it includes vbatch.hip
# whole, so its compile time is that file's own.
DEVBLOCKS_VB = "vb"
DEVBLOCKS_VB_UNITS = [("devblocks_vbatch.hip", [], "vbatch")]
# The threshold-aggregation kernels (tests/test_gpu_threshold.py) are a sixth harness,
# libhbls_devblocksta.so, on the vb harness's terms: one unit, which compiles the product's
# threshold.hip itself (fp.h's default lanes; threshold.hip sets its own HB_FAST_FPMUL).  Not split:
# it includes threshold.hip whole, so its compile time is that file's own.
DEVBLOCKS_TA = "ta"
DEVBLOCKS_TA_UNITS = [("devblocks_threshold.hip", [], "threshold")]
# the product sources a harness's units compile themselves, hashed into that harness's id
DEVBLOCKS_PRODUCT_SOURCES = {DEVBLOCKS_CURVE: ["msm.hip"], DEVBLOCKS_HASH: ["hashsplit.hip"],
                             DEVBLOCKS_PAIR: ["pipeline.hip", "vgroup.hip"], DEVBLOCKS_VB: ["vbatch.hip"],
                             DEVBLOCKS_TA: ["threshold.hip"]}
# the harnesses with a library and an id of their own, next to the block builds
DEVBLOCKS_OWN = {DEVBLOCKS_CURVE: DEVBLOCKS_CURVE_UNITS, DEVBLOCKS_HASH: DEVBLOCKS_HASH_UNITS,
                 DEVBLOCKS_PAIR: DEVBLOCKS_PAIR_UNITS, DEVBLOCKS_VB: DEVBLOCKS_VB_UNITS,
                 DEVBLOCKS_TA: DEVBLOCKS_TA_UNITS}


def devblocks_units(build: str) -> list:
    return DEVBLOCKS_OWN.get(build, DEVBLOCKS_UNITS)


def devblocks_flags(build: str) -> list:
    return [] if build in DEVBLOCKS_OWN else DEVBLOCKS_BUILDS[build]


def devblocks_path(build: str, root: str = "") -> str:
    return os.path.join(root or ROOT, "tests", "native", f"libhbls_devblocks{build}.so")


def devblocks_build_id(build: str = "64", root: str = "") -> str:
    """The id embedded in a device block harness (tests/native/devblocks*: the GPU twin of the CPU
    harness, tests/test_gpu_blocks.py, tests/test_gpu_curve.py, tests/test_gpu_hash.py, tests/test_gpu_pairing.py,
    tests/test_gpu_vbatch.py, tests/test_gpu_threshold.py): sha256 (16 hex
    digits) over the harness sources, every header of charon_amd/csrc and the flags of that build --
    what its `db_build_id()` returns.  The block builds ("64", "128") hash every
    tests/native/devblocks* file but the sources of the curve, hash, pair, vb and ta harnesses; each of those
    hashes its own sources, the shared devblocks*.h and the product sources its units compile
    themselves (DEVBLOCKS_PRODUCT_SOURCES)."""
    import hashlib
    root = root or ROOT
    csrc, native = os.path.join(root, "charon_amd", "csrc"), os.path.join(root, "tests", "native")
    own_src = {u[0] for units in DEVBLOCKS_OWN.values() for u in units}
    mine = sorted(f for f in os.listdir(native) if f.startswith("devblocks") and f.endswith((".hip", ".h")))
    if build in DEVBLOCKS_OWN:
        mine = [f for f in mine if f.endswith(".h")] + sorted({u[0] for u in DEVBLOCKS_OWN[build]})
    else:
        mine = [f for f in mine if f not in own_src]
    files = [os.path.join(native, f) for f in mine] + \
        sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h"))
    if build in DEVBLOCKS_OWN:
        files += [os.path.join(csrc, f) for f in DEVBLOCKS_PRODUCT_SOURCES[build]]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    tag = [build] if build in DEVBLOCKS_OWN else []
    h.update(" ".join(DEVBLOCKS_FLAGS + devblocks_flags(build) + [d for u in devblocks_units(build) for d in u[1]] + tag).encode())
    return DEVBLOCKS_PREFIX + h.hexdigest()[:16]


def embedded_devblocks_id(path: str) -> str:
    """The harness id inside a built device block harness, read from its bytes (no loading)."""
    import re
    with open(path, "rb") as f:
        m = re.search(rb"hbls-devblocks:[0-9a-f]{16}", f.read())
    return m.group(0).decode() if m else ""


def build_devblocks(force: bool = False, verbose: bool = True, builds=None) -> dict:
    """The builds of the device block harness, {"64": path, "128": path} (builds: others, e.g.
    [DEVBLOCKS_CURVE]).  A harness whose embedded id equals this tree's is reused; any other -- a
    header touched, other flags -- is rebuilt.  The translation units of all builds compile in
    parallel (as build_library's); a unit's time is printed, so that one slower than pipeline.hip
    shows (split it then)."""
    builds = list(builds if builds is not None else DEVBLOCKS_BUILDS)
    ids = {b: devblocks_build_id(b) for b in builds}
    paths = {b: devblocks_path(b) for b in builds}
    todo = [b for b in builds
            if force or not os.path.exists(paths[b]) or embedded_devblocks_id(paths[b]) != ids[b]]
    if not todo:
        if verbose:
            print(f"reused {', '.join(paths.values())}")
        return paths
    objdir = os.path.join(HERE, "lib", "devblocks")
    os.makedirs(objdir, exist_ok=True)
    t0 = time.time()
    jobs = []
    for b in todo:
        for src, defs, name in devblocks_units(b):
            obj = os.path.join(objdir, f"{name}_{b}.o")
            cmd = [HIPCC] + DEVBLOCKS_FLAGS + devblocks_flags(b) + defs + \
                [f'-DDB_BUILD_ID="{ids[b]}"', "-c", os.path.join(ROOT, "tests", "native", src), "-o", obj]
            jobs.append((b, name, obj, subprocess.Popen(cmd)))
    pending, took = list(jobs), {}
    while pending:  # note when each unit finishes
        for j in list(pending):
            if j[3].poll() is not None:
                took[(j[0], j[1])] = time.time() - t0
                pending.remove(j)
        if time.time() - t0 > 3000:
            for j in pending:
                j[3].kill()
            raise RuntimeError("hipcc timed out on the device block harness")
        time.sleep(0.2)
    if any(j[3].returncode != 0 for j in jobs):
        raise RuntimeError("hipcc failed on the device block harness")
    for b in todo:
        objs = [j[2] for j in jobs if j[0] == b]
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", paths[b] + ".tmp"] + objs +
                       ["-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
        os.replace(paths[b] + ".tmp", paths[b])
    if verbose:
        units = ", ".join(f"{src}/{b} {s:.0f}s" for (b, src), s in sorted(took.items()))
        print(f"built {', '.join(paths[b] for b in todo)} in {time.time() - t0:.1f}s ({units})")
    return paths


WIDEDEV_PREFIX = "hbls-widedev:"


def widedev_build_id(root: str = "") -> str:
    """The id embedded in the ladder-table device harness (tests/native/widedev.hip,
    tests/test_gpu_key_wide.py; `wd_build_id()`): sha256 over its source, the device harnesses'
    shared devblocks.h, every header of charon_amd/csrc and the flags."""
    import hashlib
    root = root or ROOT
    csrc, native = os.path.join(root, "charon_amd", "csrc"), os.path.join(root, "tests", "native")
    h = hashlib.sha256()
    for f in [os.path.join(native, "widedev.hip"), os.path.join(native, "devblocks.h")] + \
            sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")):
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(DEVBLOCKS_FLAGS).encode())
    return WIDEDEV_PREFIX + h.hexdigest()[:16]


def build_widedev(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_widedev.so: the learned keys' ladder tables and the ladders through them
    on the device, a harness of its own like the curve and hash harnesses (one unit, fp.h's default
    HB_ARG_LANES); test-only.  Reused when its embedded id equals the tree's."""
    import re
    src = os.path.join(ROOT, "tests", "native", "widedev.hip")
    out = os.path.join(ROOT, "tests", "native", "libhbls_widedev.so")
    bid = widedev_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-widedev:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    t0 = time.time()
    subprocess.run([HIPCC] + DEVBLOCKS_FLAGS + [f'-DWD_BUILD_ID="{bid}"', "-shared", "-o", out + ".tmp", src,
                                                "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=3000)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out} in {time.time() - t0:.1f}s")
    return out


SUBGDEV_PREFIX = "hbls-subgdev:"


def subgdev_build_id(root: str = "") -> str:
    """The id embedded in the batched subgroup test's device harness (tests/native/subgdev.hip,
    tests/test_gpu_subgroup_batch.py; `sd_build_id()`): sha256 over its source, the device
    harnesses' shared devblocks.h, the product source it compiles (msm.hip), every header of
    charon_amd/csrc and the flags."""
    import hashlib
    root = root or ROOT
    csrc, native = os.path.join(root, "charon_amd", "csrc"), os.path.join(root, "tests", "native")
    h = hashlib.sha256()
    for f in [os.path.join(native, "subgdev.hip"), os.path.join(native, "devblocks.h"), os.path.join(csrc, "msm.hip")] + \
            sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")):
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(DEVBLOCKS_FLAGS).encode())
    return SUBGDEV_PREFIX + h.hexdigest()[:16]


def build_subgdev(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_subgdev.so: the batched subgroup test's class sums and weighted sums on
    the device over explicit buckets, a harness of its own like build_widedev; test-only.  Reused
    when its embedded id equals the tree's."""
    import re
    src = os.path.join(ROOT, "tests", "native", "subgdev.hip")
    out = os.path.join(ROOT, "tests", "native", "libhbls_subgdev.so")
    bid = subgdev_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-subgdev:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    t0 = time.time()
    subprocess.run([HIPCC] + DEVBLOCKS_FLAGS + [f'-DSD_BUILD_ID="{bid}"', "-shared", "-o", out + ".tmp", src,
                                                "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=3000)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out} in {time.time() - t0:.1f}s")
    return out


DUTYSETDEV_PREFIX = "hbls-dutysetdev:"


def dutysetdev_build_id(root: str = "") -> str:
    """The id embedded in the set-atomic adds' device harness (tests/native/dutysetdev.hip,
    tests/test_gpu_duty_sets_kernels.py; `dsd_build_id()`): sha256 over its source, the device
    harnesses' shared devblocks.h, the product source it compiles (duty.hip), every header of
    charon_amd/csrc and the flags."""
    import hashlib
    root = root or ROOT
    csrc, native = os.path.join(root, "charon_amd", "csrc"), os.path.join(root, "tests", "native")
    h = hashlib.sha256()
    for f in [os.path.join(native, "dutysetdev.hip"), os.path.join(native, "devblocks.h"), os.path.join(csrc, "duty.hip")] + \
            sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")):
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(DEVBLOCKS_FLAGS).encode())
    return DUTYSETDEV_PREFIX + h.hexdigest()[:16]


def build_dutysetdev(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_dutysetdev.so: k_duty_set_first, k_duty_gate and k_duty_store behind the
    gate on the device over explicit words, a harness of its own like build_subgdev; test-only.
    Reused when its embedded id equals the tree's."""
    import re
    src = os.path.join(ROOT, "tests", "native", "dutysetdev.hip")
    out = os.path.join(ROOT, "tests", "native", "libhbls_dutysetdev.so")
    bid = dutysetdev_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-dutysetdev:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    t0 = time.time()
    subprocess.run([HIPCC] + DEVBLOCKS_FLAGS + [f'-DDSD_BUILD_ID="{bid}"', "-shared", "-o", out + ".tmp", src,
                                                "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=3000)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out} in {time.time() - t0:.1f}s")
    return out


DUTYFIRSTCHECK_PREFIX = "hbls-dutyfirstcheck:"
DUTYFIRSTCHECK_HEADERS = ("dutyfirst.h", "hduty.h", "hslot.h", "hgroup.h", "msgtable.h")


def dutyfirstcheck_build_id(root: str = "") -> str:
    """The id embedded in the first-error set adds' harness (tests/native/dutyfirstcheck.cpp,
    `df_build_id()`): sha256 over its source, the headers it compiles and the flags."""
    import hashlib
    root = root or ROOT
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "dutyfirstcheck.cpp")] + \
            [os.path.join(root, "charon_amd", "csrc", f) for f in DUTYFIRSTCHECK_HEADERS]:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return DUTYFIRSTCHECK_PREFIX + h.hexdigest()[:16]


def build_dutyfirstcheck(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_dutyfirstcheck.so (tests/test_duty_first_host.py): the host side of
    hbls_duty_add_sets_first on the CPU -- the set-major plan and the descent rule of the segmented
    first-error verification; test-only.  Reused when its embedded id equals the tree's, as
    build_dutycheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "dutyfirstcheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_dutyfirstcheck.so")
    bid = dutyfirstcheck_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-dutyfirstcheck:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DDF_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


DUTYFIRSTDEV_PREFIX = "hbls-dutyfirstdev:"


def dutyfirstdev_build_id(root: str = "") -> str:
    """The id embedded in the first-error set adds' device harness (tests/native/dutyfirstdev.hip,
    tests/test_gpu_duty_first_kernels.py; `dfd_build_id()`): sha256 over its source, the device
    harnesses' shared devblocks.h, the product source it compiles (dutyfirst.hip), every header of
    charon_amd/csrc and the flags."""
    import hashlib
    root = root or ROOT
    csrc, native = os.path.join(root, "charon_amd", "csrc"), os.path.join(root, "tests", "native")
    h = hashlib.sha256()
    for f in [os.path.join(native, "dutyfirstdev.hip"), os.path.join(native, "devblocks.h"),
              os.path.join(csrc, "dutyfirst.hip")] + \
            sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")):
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(DEVBLOCKS_FLAGS).encode())
    return DUTYFIRSTDEV_PREFIX + h.hexdigest()[:16]


def build_dutyfirstdev(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_dutyfirstdev.so: the kernels of the segmented first-error verification on
    the device over explicit bytes, a harness of its own like build_dutysetdev; test-only.  Reused
    when its embedded id equals the tree's."""
    import re
    src = os.path.join(ROOT, "tests", "native", "dutyfirstdev.hip")
    out = os.path.join(ROOT, "tests", "native", "libhbls_dutyfirstdev.so")
    bid = dutyfirstdev_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-dutyfirstdev:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    t0 = time.time()
    subprocess.run([HIPCC] + DEVBLOCKS_FLAGS + [f'-DDFD_BUILD_ID="{bid}"', "-shared", "-o", out + ".tmp", src,
                                                "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=3000)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out} in {time.time() - t0:.1f}s")
    return out


CLUSTERCHECK_PREFIX = "hbls-clustercheck:"
CLUSTERCHECK_HEADERS = ("cluster.h",)


def clustercheck_build_id(root: str = "") -> str:
    """The id embedded in the cluster handles' harness (tests/native/clustercheck.cpp,
    `cc_build_id()`): sha256 over its source, the header it compiles and the flags."""
    import hashlib
    root = root or ROOT
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "clustercheck.cpp")] + \
            [os.path.join(root, "charon_amd", "csrc", f) for f in CLUSTERCHECK_HEADERS]:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return CLUSTERCHECK_PREFIX + h.hexdigest()[:16]


def build_clustercheck(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_clustercheck.so (tests/test_cluster_host.py): the key rule of a cluster
    handle (cluster.h cluster_key) on the CPU; test-only.  Reused when its embedded id equals the
    tree's, as build_dutysetcheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "clustercheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_clustercheck.so")
    bid = clustercheck_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-clustercheck:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DCC_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


CLUSTERDEV_PREFIX = "hbls-clusterdev:"


def clusterdev_build_id(root: str = "") -> str:
    """The id embedded in the cluster handles' device harness (tests/native/clusterdev.hip,
    tests/test_gpu_cluster_kernels.py; `cd_build_id()`): sha256 over its source, the device
    harnesses' shared devblocks.h, the product source it compiles (cluster.hip), every header of
    charon_amd/csrc and the flags."""
    import hashlib
    root = root or ROOT
    csrc, native = os.path.join(root, "charon_amd", "csrc"), os.path.join(root, "tests", "native")
    h = hashlib.sha256()
    for f in [os.path.join(native, "clusterdev.hip"), os.path.join(native, "devblocks.h"), os.path.join(csrc, "cluster.hip")] + \
            sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")):
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(DEVBLOCKS_FLAGS).encode())
    return CLUSTERDEV_PREFIX + h.hexdigest()[:16]


def build_clusterdev(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_clusterdev.so: k_cluster_keys and k_cluster_wide on the device over
    explicit words, a harness of its own like build_dutysetdev; test-only.  Reused when its embedded
    id equals the tree's."""
    import re
    src = os.path.join(ROOT, "tests", "native", "clusterdev.hip")
    out = os.path.join(ROOT, "tests", "native", "libhbls_clusterdev.so")
    bid = clusterdev_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-clusterdev:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    t0 = time.time()
    subprocess.run([HIPCC] + DEVBLOCKS_FLAGS + [f'-DCD_BUILD_ID="{bid}"', "-shared", "-o", out + ".tmp", src,
                                                "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=3000)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out} in {time.time() - t0:.1f}s")
    return out


LOCKCHECKHOST_PREFIX = "hbls-lockcheckhost:"
LOCKCHECKHOST_HEADERS = ("lockcheck.h",)


def lockcheckhost_build_id(root: str = "") -> str:
    """The id embedded in the lock check's harness (tests/native/lockcheckhost.cpp, `lk_build_id()`):
    sha256 over its source, the header it compiles and the flags."""
    import hashlib
    root = root or ROOT
    h = hashlib.sha256()
    for f in [os.path.join(root, "tests", "native", "lockcheckhost.cpp")] + \
            [os.path.join(root, "charon_amd", "csrc", f) for f in LOCKCHECKHOST_HEADERS]:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HOSTCHECK_FLAGS).encode())
    return LOCKCHECKHOST_PREFIX + h.hexdigest()[:16]


def build_lockcheckhost(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_lockcheckhost.so (tests/test_lock_check_host.py): the rule of
    hbls_cluster_check (lockcheck.h: the signed binomial coefficients, their bit length, the plan) on
    the CPU; test-only.  Reused when its embedded id equals the tree's, as build_clustercheck."""
    import re
    src = os.path.join(ROOT, "tests", "native", "lockcheckhost.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_lockcheckhost.so")
    bid = lockcheckhost_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-lockcheckhost:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    cmd = ["g++"] + HOSTCHECK_FLAGS + [f'-DLK_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


LOCKCHECKDEV_PREFIX = "hbls-lockcheckdev:"


def lockcheckdev_build_id(root: str = "") -> str:
    """The id embedded in the lock check's device harness (tests/native/lockcheckdev.hip,
    tests/test_gpu_lock_check_kernels.py; `ld_build_id()`): sha256 over its source, the device
    harnesses' shared devblocks.h, the product source it compiles (lockcheck.hip), every header of
    charon_amd/csrc and the flags."""
    import hashlib
    root = root or ROOT
    csrc, native = os.path.join(root, "charon_amd", "csrc"), os.path.join(root, "tests", "native")
    h = hashlib.sha256()
    for f in [os.path.join(native, "lockcheckdev.hip"), os.path.join(native, "devblocks.h"),
              os.path.join(csrc, "lockcheck.hip")] + \
            sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")):
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(DEVBLOCKS_FLAGS).encode())
    return LOCKCHECKDEV_PREFIX + h.hexdigest()[:16]


def build_lockcheckdev(force: bool = False, verbose: bool = True) -> str:
    """tests/native/libhbls_lockcheckdev.so: k_lock_check and k_lock_fold on the device over the
    test's keys and statuses, a harness of its own like build_clusterdev; test-only.  Reused when its
    embedded id equals the tree's."""
    import re
    src = os.path.join(ROOT, "tests", "native", "lockcheckdev.hip")
    out = os.path.join(ROOT, "tests", "native", "libhbls_lockcheckdev.so")
    bid = lockcheckdev_build_id()
    if not force and os.path.exists(out):
        with open(out, "rb") as f:
            m = re.search(rb"hbls-lockcheckdev:[0-9a-f]{16}", f.read())
        if m and m.group(0).decode() == bid:
            return out
    t0 = time.time()
    subprocess.run([HIPCC] + DEVBLOCKS_FLAGS + [f'-DLD_BUILD_ID="{bid}"', "-shared", "-o", out + ".tmp", src,
                                                "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=3000)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out} in {time.time() - t0:.1f}s")
    return out


def build_devblocks_curve(force: bool = False, verbose: bool = True) -> str:
    """The curve harness (tests/test_gpu_curve.py), built and reused as build_devblocks' builds."""
    return build_devblocks(force, verbose, builds=[DEVBLOCKS_CURVE])[DEVBLOCKS_CURVE]


def build_devblocks_hash(force: bool = False, verbose: bool = True) -> str:
    """The hash-to-curve harness (tests/test_gpu_hash.py), built and reused as build_devblocks' builds."""
    return build_devblocks(force, verbose, builds=[DEVBLOCKS_HASH])[DEVBLOCKS_HASH]


def build_devblocks_pair(force: bool = False, verbose: bool = True) -> str:
    """The pair harness (tests/test_gpu_pairing.py), built and reused as build_devblocks' builds."""
    return build_devblocks(force, verbose, builds=[DEVBLOCKS_PAIR])[DEVBLOCKS_PAIR]


def build_devblocks_vb(force: bool = False, verbose: bool = True) -> str:
    """The vb harness (tests/test_gpu_vbatch.py), built and reused as build_devblocks' builds."""
    return build_devblocks(force, verbose, builds=[DEVBLOCKS_VB])[DEVBLOCKS_VB]


def build_devblocks_ta(force: bool = False, verbose: bool = True) -> str:
    """The ta harness (tests/test_gpu_threshold.py), built and reused as build_devblocks' builds."""
    return build_devblocks(force, verbose, builds=[DEVBLOCKS_TA])[DEVBLOCKS_TA]


def build_devblocks_all(force: bool = False, verbose: bool = True) -> dict:
    """The block harnesses and the curve, hash, pair, vb and ta harnesses, their units compiled side by side"""
    return build_devblocks(force, verbose, builds=list(DEVBLOCKS_BUILDS) + list(DEVBLOCKS_OWN))


SANITIZED_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                   "-fno-sanitize-recover=undefined", "-std=c++17", "-pthread", "-shared", "-fPIC"]


def build_hostcheck_sanitized(force: bool = False, verbose: bool = True) -> str:
    """The test harness under AddressSanitizer + UndefinedBehaviorSanitizer (host code only; the
    GPU build has no sanitizer here).  tests/test_sanitizers.py runs the host tests against it.
    Reused only when its embedded id matches the tree (as build_hostcheck)."""
    src = os.path.join(ROOT, "tests", "native", "hostcheck.cpp")
    out = os.path.join(ROOT, "tests", "native", "libhbls_hostcheck_asan.so")
    bid = hostcheck_build_id(flags=SANITIZED_FLAGS)
    if not force and os.path.exists(out) and embedded_hostcheck_id(out) == bid:
        return out
    cmd = ["g++"] + SANITIZED_FLAGS + [f'-DHC_BUILD_ID="{bid}"', "-o", out + ".tmp", src]
    subprocess.run(cmd, check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out}")
    return out


def main(argv=None):
    force = "--force" in (argv or sys.argv[1:])
    build_library(force)
    build_hostcheck(force)
    build_test_extras(force)


def build_test_extras(force: bool = False, verbose: bool = True) -> list:
    """The test-only artefacts the product does not depend on (the C client of the ABI, the device
    block harness): a failure to build one is printed and returned, never raised."""
    failed = []
    for fn in (build_c_client, build_widecheck, build_taselcheck, build_slothostcheck, build_dutycheck, build_subgcheck, build_devblocks_all, build_widedev,
               build_subgdev, build_dutysetcheck, build_dutysetdev, build_dutyfirstcheck, build_dutyfirstdev,
               build_clustercheck, build_clusterdev, build_lockcheckhost, build_lockcheckdev):
        try:
            fn(force, verbose)
        except Exception as e:  # noqa: BLE001 -- a compiler missing, a harness that does not compile
            print(f"WARNING: {fn.__name__} failed ({type(e).__name__}: {e}); the tests that need it will fail")
            failed.append(fn.__name__)
    return failed


if __name__ == "__main__":
    main()
