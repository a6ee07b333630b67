"""Build libhipbls.so (gfx950) in-tree, plus the test-only harnesses: the single-file CPU and device
harnesses (the HARNESSES table), the C client and the multi-unit device block harnesses.

    python -m charon_amd.build            # product library + test harnesses
The product library is compiled by hipcc for --offload-arch=gfx950 only.  A new single-file harness
is a row of HARNESSES: its id, its build and its place in build_test_extras follow from the row.
Rows added since that table's names were pinned by its test are MORE_HARNESSES, on the same terms.
"""

from __future__ import annotations

import collections
import functools
import hashlib
import os
import re
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

# The single-file test harnesses, in the order they are built.  From the name follow the source
# (tests/native/<name>.cpp for g++, .hip for hipcc), the output (tests/native/libhbls_<name>.so) and
# the id's prefix (hbls-<name>:).  stem: the build passes -D<STEM>_BUILD_ID="<id>" and the harness
# exports <stem>_build_id().  headers: the charon_amd/csrc headers hashed into the id -- ALL of
# them, or exactly the ones the source includes, in this order (tests/test_harness_table.py holds
# each list to the compiler's own include list).  sources: the product sources a device harness
# compiles itself, hashed too, after the device harnesses' shared devblocks.h.
HOST, DEVICE, ALL = "host", "device", "all"
Harness = collections.namedtuple("Harness", "kind stem headers sources what")
HARNESSES = {
    "hostcheck": Harness(HOST, "HC", ALL, (), "the kernels' arithmetic on the CPU: cpu_baseline and the host tests"),
    "widecheck": Harness(HOST, "WC", ALL, (), "the learned keys' ladder tables and the ladders through them on the CPU"),
    "taselcheck": Harness(HOST, "TS", ("tasel.h",), (), "the verified-member selection rule of hbls_slot_select_device"),
    "slothostcheck": Harness(HOST, "HS", ("hslot.h", "hgroup.h", "msgtable.h", "tasel.h"), (),
                             "the host plan of hbls_slot_select_batch and its matching rule"),
    "dutycheck": Harness(HOST, "DC", ("dutysel.h", "hduty.h", "hslot.h", "hgroup.h", "msgtable.h", "tasel.h"), (),
                         "the storing and firing rule of a duty session and the host plan of hbls_duty_add"),
    "subgcheck": Harness(HOST, "SG", ("subgbatch.h", "sha256.h", "hd.h", "vplan.h"), (),
                         "the batched subgroup test's digits and its plan"),
    "widedev": Harness(DEVICE, "WD", ALL, (), "the learned keys' ladder tables and the ladders through them on the device"),
    "subgdev": Harness(DEVICE, "SD", ALL, ("msm.hip",),
                       "the batched subgroup test's class sums and weighted sums over explicit buckets"),
    "dutysetcheck": Harness(HOST, "DS", ("dutysel.h", "hduty.h", "hslot.h", "hgroup.h", "msgtable.h"), (),
                            "the host side of hbls_duty_add_sets: set_off, set ids, the merge, admission, storing"),
    "dutysetdev": Harness(DEVICE, "DSD", ALL, ("duty.hip",),
                          "k_duty_set_first, k_duty_gate and k_duty_store behind the gate over explicit words"),
    "dutyfirstcheck": Harness(HOST, "DF", ("dutyfirst.h", "hduty.h", "hslot.h", "hgroup.h", "msgtable.h"), (),
                              "the host side of hbls_duty_add_sets_first: the set-major plan and the descent rule"),
    "dutyfirstdev": Harness(DEVICE, "DFD", ALL, ("dutyfirst.hip",),
                            "the kernels of the segmented first-error verification over explicit bytes"),
    "clustercheck": Harness(HOST, "CC", ("cluster.h",), (), "the key rule of a cluster handle (cluster_key)"),
    "clusterdev": Harness(DEVICE, "CD", ALL, ("cluster.hip",), "k_cluster_keys and k_cluster_wide over explicit words"),
    "lockcheckhost": Harness(HOST, "LK", ("lockcheck.h",), (),
                             "the rule of hbls_cluster_check: signed binomial coefficients, their bit length, the plan"),
    "lockcheckdev": Harness(DEVICE, "LD", ALL, ("lockcheck.hip",), "k_lock_check and k_lock_fold over the test's keys"),
}
# Rows under the same recipe that came after tests/test_harness_table.py pinned HARNESSES' names and its
# build order (that test also owns every source directly under tests/native): their sources are
# tests/native/more/<name>.cpp / .hip, their outputs and ids as the table's, and build_more_harnesses
# builds them behind build_test_extras.  tests/test_harness_more.py holds them to the table's terms.
MORE_HARNESSES = {
    "clusterselcheck": Harness(HOST, "CS", ("clustersel.h",), (),
                               "the selection rule of hbls_cluster_verify_aggregate: the selected entries, the call errors"),
    "clustersumdev": Harness(DEVICE, "CSD", ALL, ("cluster.hip",), "k_cluster_row_sum over the test's keys"),
}


def harness_row(name: str) -> Harness:
    return HARNESSES[name] if name in HARNESSES else MORE_HARNESSES[name]


def _csrc_headers(root: str) -> list:
    csrc = os.path.join(root, "charon_amd", "csrc")
    return sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h"))


def _files_id(prefix: str, files, root: str, flags) -> str:
    """prefix + sha256 (16 hex digits) over each file's root-relative path and bytes, then the flags."""
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(flags).encode())
    return prefix + h.hexdigest()[:16]


def harness_source(name: str, root: str = "") -> str:
    sub = () if name in HARNESSES else ("more",)
    return os.path.join(root or ROOT, "tests", "native", *sub, name + (".hip" if harness_row(name).kind == DEVICE else ".cpp"))


def harness_path(name: str) -> str:
    return os.path.join(ROOT, "tests", "native", f"libhbls_{name}.so")


def harness_build_id(name: str, root: str = "", defines=(), flags=None) -> str:
    """The id embedded in a harness of the table, what its `<stem>_build_id()` returns when it was
    built from this tree: over its source, for a device harness devblocks.h and its product sources,
    its csrc headers, the compiler flags (flags: another set, e.g. SANITIZED_FLAGS) and the defines."""
    root = root or ROOT
    h, csrc = harness_row(name), os.path.join(root, "charon_amd", "csrc")
    files = [harness_source(name, root)]
    if h.kind == DEVICE:
        files += [os.path.join(root, "tests", "native", "devblocks.h")] + [os.path.join(csrc, f) for f in h.sources]
    files += _csrc_headers(root) if h.headers == ALL else [os.path.join(csrc, f) for f in h.headers]
    flags = flags or (DEVBLOCKS_FLAGS if h.kind == DEVICE else HOSTCHECK_FLAGS)
    return _files_id(f"hbls-{name}:", files, root, flags + ["-D" + d for d in defines])


def embedded_harness_id(path: str, name: str) -> str:
    """The id inside a built harness file, read from its bytes (no loading); "" if it has none."""
    with open(path, "rb") as f:
        m = re.search(rb"hbls-" + name.encode() + rb":[0-9a-f]{16}", f.read())
    return m.group(0).decode() if m else ""


def build_harness(name: str, force: bool = False, verbose: bool = True, defines=(), out: str = "") -> str:
    """Build a harness of the table; test-only.  One whose embedded id equals this tree's is reused;
    any other -- a hashed file touched, other flags -- is rebuilt.  defines / out: another build of
    it (e.g. hostcheck with ("HB_HOST_MUL28",): the 28-bit host products)."""
    h, src, out = harness_row(name), harness_source(name), out or harness_path(name)
    bid = harness_build_id(name, defines=defines)
    if not force and os.path.exists(out) and embedded_harness_id(out, name) == bid:
        return out
    t0 = time.time()
    stamp = ["-D" + d for d in defines] + [f'-D{h.stem}_BUILD_ID="{bid}"']
    if h.kind == DEVICE:
        subprocess.run([HIPCC] + DEVBLOCKS_FLAGS + stamp + ["-shared", "-o", out + ".tmp", src, "-Wl,-rpath,/opt/rocm/lib"],
                       check=True, timeout=3000)
    else:
        subprocess.run(["g++"] + HOSTCHECK_FLAGS + stamp + ["-o", out + ".tmp", src], check=True, timeout=900)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"built {out} in {time.time() - t0:.1f}s" if h.kind == DEVICE else f"built {out}")
    return out


# build_<name>(force=False, verbose=True) and <name>_build_id(root="") of every harness of the table
for _name in list(HARNESSES) + list(MORE_HARNESSES):
    globals()["build_" + _name] = functools.partial(build_harness, _name)
    globals()[_name + "_build_id"] = functools.partial(harness_build_id, _name)
embedded_hostcheck_id = functools.partial(embedded_harness_id, name="hostcheck")


def hostcheck_build_id(defines=(), flags=None, root: str = "") -> str:
    """harness_build_id("hostcheck") with the defines first, as its callers pass them."""
    return harness_build_id("hostcheck", root, defines, flags)


def check_hostcheck(path: str, defines=(), root: str = "") -> str:
    """The harness's id if it was built from the tree's sources (with these defines), else raise:
    a stale harness would time or check code the kernels no longer run."""
    got, want = embedded_hostcheck_id(path), hostcheck_build_id(defines, root=root)
    if got != want:
        raise RuntimeError(f"stale CPU harness {path}: built as {got or '(unstamped)'}, the tree is {want}")
    return got


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
    root = root or ROOT
    csrc, native = os.path.join(root, "charon_amd", "csrc"), os.path.join(root, "tests", "native")
    own_src = {u[0] for units in DEVBLOCKS_OWN.values() for u in units}
    mine = sorted(f for f in os.listdir(native) if f.startswith("devblocks") and f.endswith((".hip", ".h")))
    if build in DEVBLOCKS_OWN:
        mine = [f for f in mine if f.endswith(".h")] + sorted({u[0] for u in DEVBLOCKS_OWN[build]})
    else:
        mine = [f for f in mine if f not in own_src]
    files = [os.path.join(native, f) for f in mine] + _csrc_headers(root)
    if build in DEVBLOCKS_OWN:
        files += [os.path.join(csrc, f) for f in DEVBLOCKS_PRODUCT_SOURCES[build]]
    tag = [build] if build in DEVBLOCKS_OWN else []
    return _files_id(DEVBLOCKS_PREFIX, files, root,
                     DEVBLOCKS_FLAGS + devblocks_flags(build) + [d for u in devblocks_units(build) for d in u[1]] + tag)


# the id inside a built device block harness, read from its bytes (no loading)
embedded_devblocks_id = functools.partial(embedded_harness_id, name="devblocks")


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


def _build_devblocks_own(which: str):
    def build_one(force: bool = False, verbose: bool = True) -> str:
        return build_devblocks(force, verbose, builds=[which])[which]
    build_one.__name__ = build_one.__qualname__ = "build_devblocks_" + which
    build_one.__doc__ = f"The {which} harness (libhbls_devblocks{which}.so), built and reused as build_devblocks' builds."
    return build_one


# build_devblocks_curve, _hash, _pair, _vb, _ta(force=False, verbose=True): one harness of DEVBLOCKS_OWN
for _name in DEVBLOCKS_OWN:
    globals()["build_devblocks_" + _name] = _build_devblocks_own(_name)


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
    build_more_harnesses(force)


def build_test_extras(force: bool = False, verbose: bool = True) -> list:
    """The test-only artefacts the product does not depend on: the C client of the ABI, then the
    table's harnesses in its order (hostcheck is the benchmark's too: its failure is raised, by the
    callers), the device block harnesses before the first single-file device harness.  One after the
    other; a failure to build one is printed and returned, never raised."""
    steps = ["c_client"] + [n for n in HARNESSES if n != "hostcheck"]
    steps.insert(steps.index("widedev"), "devblocks_all")
    return _build_steps(steps, force, verbose)


def build_more_harnesses(force: bool = False, verbose: bool = True) -> list:
    """MORE_HARNESSES in its order, on build_test_extras' terms (it runs behind it)."""
    return _build_steps(list(MORE_HARNESSES), force, verbose)


def _build_steps(steps, force: bool, verbose: bool) -> list:
    failed = []
    for fn in ("build_" + s for s in steps):
        try:
            globals()[fn](force, verbose)
        except Exception as e:  # noqa: BLE001 -- a compiler missing, a harness that does not compile
            print(f"WARNING: {fn} failed ({type(e).__name__}: {e}); the tests that need it will fail")
            failed.append(fn)
    return failed


if __name__ == "__main__":
    main()
