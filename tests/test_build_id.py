"""Build provenance: libhipbls.so carries the hash of the sources it was built from
(hbls_build_id), charon_amd/build.py reuses a library only when that hash matches the tree, and the
loader refuses a library built from other sources (a stale .so next to edited kernels)."""
import os
import shutil

import pytest

from charon_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _copy_tree(tmp_path):
    shutil.copytree(os.path.join(ROOT, "charon_amd", "csrc"), tmp_path / "charon_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    return str(tmp_path)


def test_source_id_tracks_every_header(tmp_path):
    root = _copy_tree(tmp_path)
    base = _lib.source_build_id(root)
    assert base == _lib.source_build_id(ROOT)
    hdr = tmp_path / "charon_amd" / "csrc" / "fp.h"
    hdr.write_text(hdr.read_text() + "\n// touched\n")
    assert _lib.source_build_id(root) != base
    (tmp_path / "include" / "hipbls.h").write_text("/* other */")
    assert len({base, _lib.source_build_id(root)}) == 2


def test_stale_library_is_refused(tmp_path):
    from charon_amd.build import build_library
    path = build_library(verbose=False)
    lib_id = _lib.embedded_build_id(path)
    assert lib_id.startswith(_lib.BUILD_ID_PREFIX)
    _lib.check_build_id(lib_id)  # the in-tree library matches the tree
    root = _copy_tree(tmp_path)
    hdr = tmp_path / "charon_amd" / "csrc" / "ec28.h"
    hdr.write_text(hdr.read_text() + "\n// touched\n")
    with pytest.raises(_lib.HipBlsUnavailable, match="stale"):
        _lib.check_build_id(lib_id, root)
    with pytest.raises(_lib.HipBlsUnavailable):
        _lib.check_build_id("hbls-build:unversioned")


def test_loaded_library_reports_its_id():
    from charon_amd.build import build_library, build_id
    L = _lib.load_library(build_library(verbose=False))
    assert L.hbls_build_id().decode() == build_id()
    # a variant build carries its defines after the hash; only the hash is compared
    _lib.check_build_id(build_id(("HB_X=1",)))


def _copy_harness_tree(tmp_path):
    root = _copy_tree(tmp_path)
    os.makedirs(tmp_path / "tests" / "native")
    shutil.copy(os.path.join(ROOT, "tests", "native", "hostcheck.cpp"), tmp_path / "tests" / "native")
    return root


def test_stale_cpu_harness_is_refused(tmp_path):
    """The g++ harness behind cpu_baseline and the host tests carries the hash of its sources and
    flags (hc_build_id); one built before a header changed is refused and rebuilt."""
    import ctypes
    from charon_amd import build
    path = build.build_hostcheck(verbose=False)
    hid = build.check_hostcheck(path)  # the in-tree harness matches the tree
    assert hid.startswith(build.HOSTCHECK_PREFIX)
    lib = ctypes.CDLL(path)
    lib.hc_build_id.restype = ctypes.c_char_p
    assert lib.hc_build_id().decode() == hid
    root = _copy_harness_tree(tmp_path)
    assert build.hostcheck_build_id(root=root) == hid
    hdr = tmp_path / "charon_amd" / "csrc" / "fp.h"
    hdr.write_text(hdr.read_text() + "\n// touched\n")
    with pytest.raises(RuntimeError, match="stale CPU harness"):
        build.check_hostcheck(path, root=root)
    # other flags or defines are another harness
    assert build.hostcheck_build_id(("HB_HOST_MUL28",)) != hid
    assert build.hostcheck_build_id(flags=build.SANITIZED_FLAGS) != hid


def test_devblocks_id_tracks_headers_and_harness(tmp_path):
    """The device block harness (tests/native/devblocks*, tests/test_gpu_blocks.py) carries the
    hash of its sources, every csrc header and its build's flags (db_build_id): touching a header
    or a harness source changes it, an unrelated file does not, and the two builds differ.  A
    harness built here carries its tree's id."""
    from charon_amd import build
    root = _copy_harness_tree(tmp_path)
    native = os.path.join(ROOT, "tests", "native")
    mine = sorted(f for f in os.listdir(native) if f.startswith("devblocks") and f.endswith((".hip", ".h")))
    assert "devblocks_leaf.hip" in mine and "devblocks_grp.hip" in mine and "devblocks.h" in mine
    for f in mine:
        shutil.copy(os.path.join(native, f), tmp_path / "tests" / "native")
    ids = {b: build.devblocks_build_id(b, root=root) for b in build.DEVBLOCKS_BUILDS}
    assert ids == {b: build.devblocks_build_id(b) for b in build.DEVBLOCKS_BUILDS}
    assert len(set(ids.values())) == 2 and all(i.startswith(build.DEVBLOCKS_PREFIX) for i in ids.values())
    # unrelated files: a product translation unit, the CPU harness, the public header, a new file
    for rel in ("charon_amd/csrc/pipeline.hip", "tests/native/hostcheck.cpp", "include/hipbls.h"):
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
    (tmp_path / "tests" / "native" / "other.hip").write_text("// other\n")
    assert build.devblocks_build_id("64", root=root) == ids["64"]
    for rel in ("charon_amd/csrc/pair28.h", "charon_amd/csrc/fp.h", "tests/native/devblocks_grp.hip",
                "tests/native/devblocks.h"):
        before = build.devblocks_build_id("128", root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id("128", root=root) != before, rel
    assert build.devblocks_build_id("64", root=root) != ids["64"]
    for b in build.DEVBLOCKS_BUILDS:  # what build() left in the tree, if it is there, is this tree's
        path = build.devblocks_path(b)
        if os.path.exists(path) and build.embedded_devblocks_id(path).startswith(build.DEVBLOCKS_PREFIX):
            assert os.path.basename(path) == f"libhbls_devblocks{b}.so"


def test_curve_harness_id_is_its_own(tmp_path):
    """The curve harness (tests/native/devblocks_curve.hip, devblocks_msm.hip; tests/test_gpu_curve.py)
    carries an id of its own: its sources, the shared devblocks.h, every csrc header and the product
    source its MSM unit compiles itself (msm.hip) change it; an unrelated file does not.  The block
    harnesses' ids do not move with a curve source or msm.hip, so they are neither stale nor rebuilt
    when only the curve layer's harness changes -- and every devblocks*.hip belongs to one of them."""
    from charon_amd import build
    root = _copy_harness_tree(tmp_path)
    native = os.path.join(ROOT, "tests", "native")
    mine = sorted(f for f in os.listdir(native) if f.startswith("devblocks") and f.endswith((".hip", ".h")))
    for f in mine:
        shutil.copy(os.path.join(native, f), tmp_path / "tests" / "native")
    curve = build.DEVBLOCKS_CURVE
    assert {u[0] for u in build.devblocks_units(curve)} == {"devblocks_curve.hip", "devblocks_msm.hip"}
    assert {u[0] for b in list(build.DEVBLOCKS_BUILDS) + [curve, build.DEVBLOCKS_HASH, build.DEVBLOCKS_PAIR, build.DEVBLOCKS_VB,
                                                        build.DEVBLOCKS_TA]
            for u in build.devblocks_units(b)} == {f for f in mine if f.endswith(".hip")}  # every source is built
    cid = build.devblocks_build_id(curve, root=root)
    assert cid == build.devblocks_build_id(curve) and cid.startswith(build.DEVBLOCKS_PREFIX)
    blocks = {b: build.devblocks_build_id(b, root=root) for b in build.DEVBLOCKS_BUILDS}
    assert cid not in blocks.values()
    for rel in ("charon_amd/csrc/pipeline.hip", "tests/native/hostcheck.cpp", "include/hipbls.h",
                "tests/native/devblocks_grp.hip", "tests/native/devblocks_leaf.hip",
                "tests/native/devblocks_h2c.hip", "tests/native/devblocks_h2c_std.hip", "charon_amd/csrc/hashsplit.hip"):
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
    assert build.devblocks_build_id(curve, root=root) == cid
    blocks = {b: build.devblocks_build_id(b, root=root) for b in build.DEVBLOCKS_BUILDS}
    for rel in ("tests/native/devblocks_curve.hip", "tests/native/devblocks_msm.hip", "charon_amd/csrc/msm.hip"):
        before = build.devblocks_build_id(curve, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(curve, root=root) != before, rel
        assert {b: build.devblocks_build_id(b, root=root) for b in build.DEVBLOCKS_BUILDS} == blocks, rel
    for rel in ("tests/native/devblocks.h", "charon_amd/csrc/ec28.h", "charon_amd/csrc/fp.h"):
        before = build.devblocks_build_id(curve, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(curve, root=root) != before, rel
    path = build.devblocks_path(curve)
    assert os.path.basename(path) == "libhbls_devblockscurve.so"
    if os.path.exists(path):  # what build() left in the tree is this tree's
        assert build.embedded_devblocks_id(path) == build.devblocks_build_id(curve)


def test_hash_harness_id_is_its_own(tmp_path):
    """The hash harness (tests/native/devblocks_h2c.hip, devblocks_h2c_std.hip; tests/test_gpu_hash.py)
    on the same terms: its sources, the shared devblocks.h, every csrc header and the product source
    its stage unit compiles itself (hashsplit.hip) change its id; an unrelated file, a block or curve
    source or msm.hip does not.  The ids of the block and curve harnesses do not move with a hash
    source or hashsplit.hip, the three kinds of id differ, and build_devblocks_all builds all of them."""
    from charon_amd import build
    root = _copy_harness_tree(tmp_path)
    native = os.path.join(ROOT, "tests", "native")
    mine = sorted(f for f in os.listdir(native) if f.startswith("devblocks") and f.endswith((".hip", ".h")))
    for f in mine:
        shutil.copy(os.path.join(native, f), tmp_path / "tests" / "native")
    hsh, curve = build.DEVBLOCKS_HASH, build.DEVBLOCKS_CURVE
    assert {u[0] for u in build.devblocks_units(hsh)} == {"devblocks_h2c.hip", "devblocks_h2c_std.hip"}
    assert len({u[2] for u in build.devblocks_units(hsh)}) == len(build.devblocks_units(hsh))  # one object each
    assert build.DEVBLOCKS_PRODUCT_SOURCES[hsh] == ["hashsplit.hip"] and build.DEVBLOCKS_PRODUCT_SOURCES[curve] == ["msm.hip"]
    others = list(build.DEVBLOCKS_BUILDS) + [curve]

    def ids(which):
        return {b: build.devblocks_build_id(b, root=root) for b in which}
    hid = build.devblocks_build_id(hsh, root=root)
    assert hid == build.devblocks_build_id(hsh) and hid.startswith(build.DEVBLOCKS_PREFIX)
    assert len(set(ids(others + [hsh]).values())) == 4  # the three harness kinds (two block builds) differ
    for rel in ("charon_amd/csrc/pipeline.hip", "charon_amd/csrc/hash.hip", "charon_amd/csrc/msm.hip",
                "tests/native/hostcheck.cpp", "include/hipbls.h", "tests/native/devblocks_grp.hip",
                "tests/native/devblocks_leaf.hip", "tests/native/devblocks_curve.hip", "tests/native/devblocks_msm.hip"):
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
    assert build.devblocks_build_id(hsh, root=root) == hid
    before_others = ids(others)
    for rel in ("tests/native/devblocks_h2c.hip", "tests/native/devblocks_h2c_std.hip", "charon_amd/csrc/hashsplit.hip"):
        before = build.devblocks_build_id(hsh, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(hsh, root=root) != before, rel
        assert ids(others) == before_others, rel
    for rel in ("tests/native/devblocks.h", "charon_amd/csrc/h2c.h", "charon_amd/csrc/sha256.h", "charon_amd/csrc/fp.h"):
        before = build.devblocks_build_id(hsh, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(hsh, root=root) != before, rel
    path = build.devblocks_path(hsh)
    assert os.path.basename(path) == "libhbls_devblockshash.so"
    if os.path.exists(path):  # what build() left in the tree is this tree's
        assert build.embedded_devblocks_id(path) == build.devblocks_build_id(hsh)
    # build() goes through build_devblocks_all: every harness is among its builds
    seen = {}
    real = build.build_devblocks
    try:
        build.build_devblocks = lambda force=False, verbose=True, builds=None: seen.setdefault("builds", list(builds))
        build.build_devblocks_all()
    finally:
        build.build_devblocks = real
    assert sorted(seen["builds"]) == sorted(others + [hsh, build.DEVBLOCKS_PAIR, build.DEVBLOCKS_VB, build.DEVBLOCKS_TA])


def test_pair_harness_id_is_its_own(tmp_path):
    """The pair harness (tests/native/devblocks_pair.hip, devblocks_vgroup.hip; tests/test_gpu_pairing.py)
    on the same terms: its two sources, the shared devblocks.h, every csrc header and the product
    sources its units compile themselves (pipeline.hip, vgroup.hip) change its id; an unrelated file or
    another harness's source does not.  The other harnesses' ids do not move with a pair source,
    pipeline.hip or vgroup.hip; all the ids differ; every devblocks*.hip belongs to exactly one
    harness (the vb harness among them); build_devblocks_all builds it."""
    from charon_amd import build
    root = _copy_harness_tree(tmp_path)
    native = os.path.join(ROOT, "tests", "native")
    mine = sorted(f for f in os.listdir(native) if f.startswith("devblocks") and f.endswith((".hip", ".h")))
    for f in mine:
        shutil.copy(os.path.join(native, f), tmp_path / "tests" / "native")
    pair = build.DEVBLOCKS_PAIR
    assert pair == "pair" and pair in build.DEVBLOCKS_OWN
    assert {u[0] for u in build.devblocks_units(pair)} == {"devblocks_pair.hip", "devblocks_vgroup.hip"}
    assert len({u[2] for u in build.devblocks_units(pair)}) == len(build.devblocks_units(pair))  # one object each
    assert build.DEVBLOCKS_PRODUCT_SOURCES[pair] == ["pipeline.hip", "vgroup.hip"]
    # pipeline.hip sets its own HB_FAST_FPMUL and HB_ARG_LANES; vgroup.hip takes the default lanes: no such flag
    assert not any("HB_ARG_LANES" in d or "HB_FAST_FPMUL" in d for u in build.devblocks_units(pair) for d in u[1])
    assert build.devblocks_flags(pair) == []
    others = list(build.DEVBLOCKS_BUILDS) + [build.DEVBLOCKS_CURVE, build.DEVBLOCKS_HASH, build.DEVBLOCKS_VB,
                                             build.DEVBLOCKS_TA]
    every = others + [pair]
    owner = {}
    for b in every:  # every source in exactly one harness (the two block builds share theirs)
        for src in {u[0] for u in build.devblocks_units(b)}:
            owner.setdefault(src, set()).add("blocks" if b in build.DEVBLOCKS_BUILDS else b)
    assert set(owner) == {f for f in mine if f.endswith(".hip")} and all(len(v) == 1 for v in owner.values())

    def ids(which):
        return {b: build.devblocks_build_id(b, root=root) for b in which}
    pid = build.devblocks_build_id(pair, root=root)
    assert pid == build.devblocks_build_id(pair) and pid.startswith(build.DEVBLOCKS_PREFIX)
    assert len(set(ids(every).values())) == 7
    for rel in ("charon_amd/csrc/hash.hip", "charon_amd/csrc/msm.hip", "charon_amd/csrc/hashsplit.hip",
                "charon_amd/csrc/vbatch.hip", "charon_amd/csrc/threshold.hip", "tests/native/devblocks_threshold.hip",
                "tests/native/hostcheck.cpp", "include/hipbls.h",
                "tests/native/devblocks_grp.hip", "tests/native/devblocks_leaf.hip", "tests/native/devblocks_curve.hip",
                "tests/native/devblocks_msm.hip", "tests/native/devblocks_h2c.hip", "tests/native/devblocks_h2c_std.hip",
                "tests/native/devblocks_vbatch.hip"):
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
    assert build.devblocks_build_id(pair, root=root) == pid
    before_others = ids(others)
    for rel in ("tests/native/devblocks_pair.hip", "tests/native/devblocks_vgroup.hip", "charon_amd/csrc/pipeline.hip",
                "charon_amd/csrc/vgroup.hip"):
        before = build.devblocks_build_id(pair, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(pair, root=root) != before, rel
        assert ids(others) == before_others, rel
    for rel in ("tests/native/devblocks.h", "charon_amd/csrc/pair28.h", "charon_amd/csrc/lines.h", "charon_amd/csrc/layout.h",
                "charon_amd/csrc/fp.h"):
        before = build.devblocks_build_id(pair, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(pair, root=root) != before, rel
    path = build.devblocks_path(pair)
    assert os.path.basename(path) == "libhbls_devblockspair.so"
    if os.path.exists(path):  # what build() left in the tree is this tree's
        assert build.embedded_devblocks_id(path) == build.devblocks_build_id(pair)
    seen = {}
    real = build.build_devblocks
    try:
        build.build_devblocks = lambda force=False, verbose=True, builds=None: seen.setdefault("builds", list(builds))
        build.build_devblocks_all()
    finally:
        build.build_devblocks = real
    assert pair in seen["builds"] and sorted(seen["builds"]) == sorted(every)


def test_vb_harness_id_is_its_own(tmp_path):
    """The vb harness (tests/native/devblocks_vbatch.hip; tests/test_gpu_vbatch.py) on the same terms:
    its one source, the shared devblocks.h, every csrc header and the product source its unit compiles
    itself (vbatch.hip) change its id; an unrelated file or another harness's source does not.
    Touching vbatch.hip moves this id (and the library's) and no other harness's; all the ids differ;
    every devblocks*.hip belongs to exactly one harness; build_devblocks_all builds it next to the
    others."""
    from charon_amd import build
    root = _copy_harness_tree(tmp_path)
    native = os.path.join(ROOT, "tests", "native")
    mine = sorted(f for f in os.listdir(native) if f.startswith("devblocks") and f.endswith((".hip", ".h")))
    for f in mine:
        shutil.copy(os.path.join(native, f), tmp_path / "tests" / "native")
    vbh = build.DEVBLOCKS_VB
    assert vbh == "vb" and vbh in build.DEVBLOCKS_OWN
    assert [u[0] for u in build.devblocks_units(vbh)] == ["devblocks_vbatch.hip"]  # one unit
    assert build.DEVBLOCKS_PRODUCT_SOURCES[vbh] == ["vbatch.hip"]
    # vbatch.hip sets its own HB_FAST_FPMUL and takes fp.h's default lanes: the build passes neither
    assert not any("HB_ARG_LANES" in d or "HB_FAST_FPMUL" in d for u in build.devblocks_units(vbh) for d in u[1])
    assert build.devblocks_flags(vbh) == []
    others = list(build.DEVBLOCKS_BUILDS) + [build.DEVBLOCKS_CURVE, build.DEVBLOCKS_HASH, build.DEVBLOCKS_PAIR]
    every = others + [vbh, build.DEVBLOCKS_TA]
    owner = {}
    for b in every:  # every source in exactly one harness (the two block builds share theirs)
        for src in {u[0] for u in build.devblocks_units(b)}:
            owner.setdefault(src, set()).add("blocks" if b in build.DEVBLOCKS_BUILDS else b)
    assert set(owner) == {f for f in mine if f.endswith(".hip")} and all(len(v) == 1 for v in owner.values())
    assert owner["devblocks_vbatch.hip"] == {vbh}

    def ids(which):
        return {b: build.devblocks_build_id(b, root=root) for b in which}
    vid = build.devblocks_build_id(vbh, root=root)
    assert vid == build.devblocks_build_id(vbh) and vid.startswith(build.DEVBLOCKS_PREFIX)
    assert len(set(ids(every).values())) == 7
    for rel in ("charon_amd/csrc/hash.hip", "charon_amd/csrc/msm.hip", "charon_amd/csrc/hashsplit.hip",
                "charon_amd/csrc/pipeline.hip", "charon_amd/csrc/vgroup.hip", "charon_amd/csrc/threshold.hip",
                "tests/native/devblocks_threshold.hip", "tests/native/hostcheck.cpp", "include/hipbls.h", "tests/native/devblocks_grp.hip",
                "tests/native/devblocks_leaf.hip", "tests/native/devblocks_curve.hip", "tests/native/devblocks_msm.hip",
                "tests/native/devblocks_h2c.hip", "tests/native/devblocks_h2c_std.hip", "tests/native/devblocks_pair.hip",
                "tests/native/devblocks_vgroup.hip"):
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
    assert build.devblocks_build_id(vbh, root=root) == vid
    before_others, lib_before = ids(others), _lib.source_build_id(root)
    for rel in ("tests/native/devblocks_vbatch.hip", "charon_amd/csrc/vbatch.hip"):
        before = build.devblocks_build_id(vbh, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(vbh, root=root) != before, rel
        assert ids(others) == before_others, rel
    assert _lib.source_build_id(root) != lib_before  # vbatch.hip is the library's too
    for rel in ("tests/native/devblocks.h", "charon_amd/csrc/rlc.h", "charon_amd/csrc/ec28.h", "charon_amd/csrc/layout.h",
                "charon_amd/csrc/sha256.h", "charon_amd/csrc/fp.h"):
        before = build.devblocks_build_id(vbh, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(vbh, root=root) != before, rel
    path = build.devblocks_path(vbh)
    assert os.path.basename(path) == "libhbls_devblocksvb.so"
    if os.path.exists(path):  # what build() left in the tree is this tree's
        assert build.embedded_devblocks_id(path) == build.devblocks_build_id(vbh)
    assert build.build_devblocks_vb.__doc__
    seen = {}
    real = build.build_devblocks
    try:
        build.build_devblocks = lambda force=False, verbose=True, builds=None: seen.setdefault("builds", list(builds))
        build.build_devblocks_all()
        assert sorted(seen["builds"]) == sorted(every)
        seen.clear()
        build.build_devblocks = lambda force=False, verbose=True, builds=None: {b: seen.setdefault("one", b) for b in builds}
        assert build.build_devblocks_vb() == vbh and seen == {"one": vbh}
    finally:
        build.build_devblocks = real


def test_ta_harness_id_is_its_own(tmp_path):
    """The ta harness (tests/native/devblocks_threshold.hip; tests/test_gpu_threshold.py) on the same
    terms: its one source, the shared devblocks.h, every csrc header and the product source its unit
    compiles itself (threshold.hip) change its id; an unrelated file or another harness's source does
    not.  Touching threshold.hip moves this id (and the library's) and no other harness's; touching
    devblocks_threshold.hip moves this id alone; all the ids differ; every devblocks*.hip belongs to
    exactly one harness; build_devblocks_all builds it next to the others."""
    from charon_amd import build
    root = _copy_harness_tree(tmp_path)
    native = os.path.join(ROOT, "tests", "native")
    mine = sorted(f for f in os.listdir(native) if f.startswith("devblocks") and f.endswith((".hip", ".h")))
    for f in mine:
        shutil.copy(os.path.join(native, f), tmp_path / "tests" / "native")
    ta = build.DEVBLOCKS_TA
    assert ta == "ta" and ta in build.DEVBLOCKS_OWN
    assert [u[0] for u in build.devblocks_units(ta)] == ["devblocks_threshold.hip"]  # one unit
    assert build.DEVBLOCKS_PRODUCT_SOURCES[ta] == ["threshold.hip"]
    # threshold.hip sets its own HB_FAST_FPMUL and takes fp.h's default lanes: the build passes neither
    assert not any("HB_ARG_LANES" in d or "HB_FAST_FPMUL" in d for u in build.devblocks_units(ta) for d in u[1])
    assert build.devblocks_flags(ta) == []
    others = list(build.DEVBLOCKS_BUILDS) + [build.DEVBLOCKS_CURVE, build.DEVBLOCKS_HASH, build.DEVBLOCKS_PAIR,
                                             build.DEVBLOCKS_VB]
    every = others + [ta]
    owner = {}
    for b in every:  # every source in exactly one harness (the two block builds share theirs)
        for src in {u[0] for u in build.devblocks_units(b)}:
            owner.setdefault(src, set()).add("blocks" if b in build.DEVBLOCKS_BUILDS else b)
    assert set(owner) == {f for f in mine if f.endswith(".hip")} and all(len(v) == 1 for v in owner.values())
    assert owner["devblocks_threshold.hip"] == {ta}

    def ids(which):
        return {b: build.devblocks_build_id(b, root=root) for b in which}
    tid = build.devblocks_build_id(ta, root=root)
    assert tid == build.devblocks_build_id(ta) and tid.startswith(build.DEVBLOCKS_PREFIX)
    assert len(set(ids(every).values())) == 7
    for rel in ("charon_amd/csrc/hash.hip", "charon_amd/csrc/msm.hip", "charon_amd/csrc/hashsplit.hip",
                "charon_amd/csrc/pipeline.hip", "charon_amd/csrc/vgroup.hip", "charon_amd/csrc/vbatch.hip",
                "charon_amd/csrc/hipbls.hip", "tests/native/hostcheck.cpp", "include/hipbls.h", "tests/native/devblocks_grp.hip",
                "tests/native/devblocks_leaf.hip", "tests/native/devblocks_curve.hip", "tests/native/devblocks_msm.hip",
                "tests/native/devblocks_h2c.hip", "tests/native/devblocks_h2c_std.hip", "tests/native/devblocks_pair.hip",
                "tests/native/devblocks_vgroup.hip", "tests/native/devblocks_vbatch.hip"):
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
    assert build.devblocks_build_id(ta, root=root) == tid
    before_others, lib_before = ids(others), _lib.source_build_id(root)
    for rel in ("tests/native/devblocks_threshold.hip", "charon_amd/csrc/threshold.hip"):
        before = build.devblocks_build_id(ta, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(ta, root=root) != before, rel
        assert ids(others) == before_others, rel
        if rel.startswith("tests/"):
            assert _lib.source_build_id(root) == lib_before  # the harness source is not the library's
    assert _lib.source_build_id(root) != lib_before  # threshold.hip is the library's too
    for rel in ("tests/native/devblocks.h", "charon_amd/csrc/ta_small.h", "charon_amd/csrc/tasel.h", "charon_amd/csrc/layout.h",
                "charon_amd/csrc/ec28.h", "charon_amd/csrc/fr.h", "charon_amd/csrc/fp.h"):
        before = build.devblocks_build_id(ta, root=root)
        with open(tmp_path / rel, "a") as f:
            f.write("\n// touched\n")
        assert build.devblocks_build_id(ta, root=root) != before, rel
    path = build.devblocks_path(ta)
    assert os.path.basename(path) == "libhbls_devblocksta.so"
    if os.path.exists(path):  # what build() left in the tree is this tree's
        assert build.embedded_devblocks_id(path) == build.devblocks_build_id(ta)
    assert build.build_devblocks_ta.__doc__
    seen = {}
    real = build.build_devblocks
    try:
        build.build_devblocks = lambda force=False, verbose=True, builds=None: seen.setdefault("builds", list(builds))
        build.build_devblocks_all()
        assert sorted(seen["builds"]) == sorted(every)
        seen.clear()
        build.build_devblocks = lambda force=False, verbose=True, builds=None: {b: seen.setdefault("one", b) for b in builds}
        assert build.build_devblocks_ta() == ta and seen == {"one": ta}
    finally:
        build.build_devblocks = real
