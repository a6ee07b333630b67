"""The table of test harnesses in charon_amd/build.py (HARNESSES): the ids it gives are the ones
every harness has carried, each entry hashes what its source really compiles, and every native
source under tests/native belongs to one build.  CPU only; nothing here compiles a harness."""
import os
import re
import shutil
import subprocess

import pytest

from charon_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HOST = ("hostcheck", "widecheck", "taselcheck", "slothostcheck", "dutycheck", "dutysetcheck", "subgcheck",
        "dutyfirstcheck", "clustercheck", "lockcheckhost")
DEVICE = ("widedev", "subgdev", "dutysetdev", "dutyfirstdev", "clusterdev", "lockcheckdev")

# the ids of the synthetic tree below, as the per-harness functions gave them before there was a table
PINNED = {
    "hostcheck": "hbls-hostcheck:1d86b441c74d62a4",
    "widecheck": "hbls-widecheck:f30cdbc6cbb0df43",
    "taselcheck": "hbls-taselcheck:be712bcb5c3f6195",
    "slothostcheck": "hbls-slothostcheck:3344c2bb55851db8",
    "dutycheck": "hbls-dutycheck:396553fe0f8799ae",
    "dutysetcheck": "hbls-dutysetcheck:d24c30c49651286f",
    "subgcheck": "hbls-subgcheck:50a688d2efdbb4eb",
    "dutyfirstcheck": "hbls-dutyfirstcheck:7f5ac44e67167ee5",
    "clustercheck": "hbls-clustercheck:d8de37f2ad67c755",
    "lockcheckhost": "hbls-lockcheckhost:959d88e5292b4ed0",
    "widedev": "hbls-widedev:ac5e78525f6f5cf1",
    "subgdev": "hbls-subgdev:90c9cf0ea6272de9",
    "dutysetdev": "hbls-dutysetdev:784b2118ef9aa419",
    "dutyfirstdev": "hbls-dutyfirstdev:61258b2c28123038",
    "clusterdev": "hbls-clusterdev:8c300a26e179cfb9",
    "lockcheckdev": "hbls-lockcheckdev:23f083e1f547ffb1",
}


def test_ids_are_pinned_on_a_synthetic_tree(tmp_path):
    """Every file's content is its own path: the ids depend on the hashing order, the paths, the
    header lists, the product sources and the flags alone -- and are the ones from before the table."""
    files = ["charon_amd/csrc/" + h + ".h" for h in
             "a b cluster dutyfirst dutysel hd hduty hgroup hslot lockcheck msgtable sha256 subgbatch tasel vplan".split()] + \
        ["charon_amd/csrc/" + s + ".hip" for s in "msm duty dutyfirst cluster lockcheck".split()] + \
        [f"tests/native/{n}.cpp" for n in HOST] + [f"tests/native/{n}.hip" for n in DEVICE] + ["tests/native/devblocks.h"]
    for rel in files:
        os.makedirs(tmp_path / os.path.dirname(rel), exist_ok=True)
        (tmp_path / rel).write_text(rel + "\n")
    root = str(tmp_path)
    assert {n: getattr(build, n + "_build_id")(root=root) for n in HOST + DEVICE} == PINNED
    assert build.hostcheck_build_id(("HB_HOST_MUL28",), root=root) == "hbls-hostcheck:d6b015bdf139d40b"
    assert build.hostcheck_build_id(flags=build.SANITIZED_FLAGS, root=root) == "hbls-hostcheck:940bdc97407f6866"


def test_the_table_is_these_harnesses_in_build_order():
    assert set(build.HARNESSES) == set(HOST + DEVICE)
    assert all(build.HARNESSES[n].kind == (build.HOST if n in HOST else build.DEVICE) for n in build.HARNESSES)
    stems = [h.stem for h in build.HARNESSES.values()]
    assert len(set(stems)) == len(stems)  # one exported <stem>_build_id each
    seen = []
    real = {n: getattr(build, n) for n in ["build_c_client", "build_devblocks_all"] + ["build_" + h for h in build.HARNESSES]}
    try:
        for n in real:
            setattr(build, n, lambda force, verbose, n=n: seen.append(n) if n != "build_subgdev" else 1 / 0)
        failed = build.build_test_extras(verbose=False)
    finally:
        for n, fn in real.items():
            setattr(build, n, fn)
    assert failed == ["build_subgdev"]  # printed and returned, and the rest is still built
    assert seen == ["build_" + n for n in
                    "c_client widecheck taselcheck slothostcheck dutycheck subgcheck devblocks_all widedev dutysetcheck "
                    "dutysetdev dutyfirstcheck dutyfirstdev clustercheck clusterdev lockcheckhost lockcheckdev".split()]


@pytest.mark.parametrize("name", [n for n in HOST if build.HARNESSES[n].headers != build.ALL])
def test_named_headers_are_what_the_source_includes(name):
    """A named list is sound only while it equals the compiler's own list of the csrc headers the
    harness compiles: one too few and a stale harness is reused, one too many and it is rebuilt for
    nothing."""
    r = subprocess.run(["g++", "-std=c++17", "-MM", build.harness_source(name)], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    csrc = os.path.join(ROOT, "charon_amd", "csrc")
    deps = [os.path.normpath(os.path.join(ROOT, d)) for d in r.stdout.replace("\\\n", " ").split()[1:]]
    included = {os.path.basename(d) for d in deps if os.path.dirname(d) == csrc and d.endswith(".h")}
    assert included == set(build.HARNESSES[name].headers)
    assert len(set(build.HARNESSES[name].headers)) == len(build.HARNESSES[name].headers)


@pytest.mark.parametrize("name", DEVICE)
def test_product_sources_are_what_the_device_source_includes(name):
    with open(build.harness_source(name)) as f:
        includes = re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    assert "devblocks.h" in includes
    assert [os.path.basename(i) for i in includes if i.endswith(".hip")] == list(build.HARNESSES[name].sources)
    assert all(i == "../../charon_amd/csrc/" + os.path.basename(i) for i in includes if i.endswith(".hip"))


@pytest.fixture
def tree(tmp_path):
    """A copy of the real sources the ids hash, for a test to append to"""
    root = tmp_path
    shutil.copytree(os.path.join(ROOT, "charon_amd", "csrc"), root / "charon_amd" / "csrc")
    os.makedirs(root / "tests" / "native")
    for n in build.HARNESSES:
        shutil.copy(build.harness_source(n), root / "tests" / "native")
    shutil.copy(os.path.join(NATIVE, "devblocks.h"), root / "tests" / "native")
    return str(root)


@pytest.mark.parametrize("name", HOST + DEVICE)
def test_id_moves_with_every_hashed_file_and_no_other(name, tree):
    h = build.HARNESSES[name]
    assert build.harness_build_id(name, root=tree) == build.harness_build_id(name)
    csrc = sorted(f for f in os.listdir(os.path.join(tree, "charon_amd", "csrc")))
    headers = [f for f in csrc if f.endswith(".h")]
    mine = headers if h.headers == build.ALL else list(h.headers)
    assert set(mine) <= set(headers)
    hashed = [os.path.relpath(build.harness_source(name, tree), tree)] + ["charon_amd/csrc/" + f for f in mine + list(h.sources)] + \
        (["tests/native/devblocks.h"] if h.kind == build.DEVICE else [])

    def touch(rel):
        before = build.harness_build_id(name, root=tree)
        with open(os.path.join(tree, rel), "a") as f:
            f.write("\n// touched\n")
        return before != build.harness_build_id(name, root=tree)
    for rel in hashed:
        assert touch(rel), rel
    unlisted = [f for f in headers if f not in mine]
    assert unlisted or h.headers == build.ALL
    others = ["charon_amd/csrc/" + f for f in unlisted + [f for f in csrc if f.endswith(".hip") and f not in h.sources]] + \
        ([] if h.kind == build.DEVICE else ["tests/native/devblocks.h"])
    for rel in others:
        assert not touch(rel), rel


def test_every_native_source_is_owned():
    """Every program source under tests/native is built by exactly one row of the table or one
    device block harness, but for the ones named here (the C client has a build of its own; the
    devcheck sources are built by hand, by build_devcheck.sh)."""
    unowned = {"cabi_client.c", "devcheck.hip", "devcheck_std.hip", "build_devcheck.sh"}
    owners = {}
    for n in build.HARNESSES:
        owners.setdefault(os.path.basename(build.harness_source(n)), []).append(n)
    for b, units in [("blocks", build.DEVBLOCKS_UNITS)] + list(build.DEVBLOCKS_OWN.items()):
        for src in {u[0] for u in units}:
            owners.setdefault(src, []).append("devblocks " + b)
    sources = {f for f in os.listdir(NATIVE) if f.endswith((".cpp", ".hip"))}
    assert sources - unowned == set(owners) and all(len(v) == 1 for v in owners.values()), owners
    assert unowned <= set(os.listdir(NATIVE)) and not unowned & set(owners)
