"""CPU: the weight packer's index maps (nerfmeshes_amd/csrc/mlp_pack.h) against recorded fingerprints.

tests/tools/mlp_pack_dump.cpp is compiled with g++ against the header (host only, no HIP) and prints, for a fixed matrix of
network descriptions -- the tuned shapes, the generic family's width classes and encodings, the bf16x3 stream, the layer-wise
image --, the size of every index map, the blob offsets, skip_mask, the encodings' chunk counts and an FNV-1a-64 of the index
(before and with the plain-copy tail).  tests/golden/mlp_pack_fingerprints.json holds what the packer printed BEFORE the
tuned and the generic family's builders were merged into one (recorded from the two separate builders, moved verbatim into a
header), so any changed entry of any index map fails here, without a GPU.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerfmeshes_amd", "csrc")

# Independent anchors: a separate transcription of the tuned packer (FD 4, skip_step 4, both inputs included, the index before
# the plain-copy tail): entries, off_bias / off_wa / off_wr / off_bwd, skip_mask, FNV-1a-64
ANCHORS = {
    "tuned H256 L8 s4 FX10 FD4 in11 v1": (1155648, [594432, 596928, 597184, 597568], 16, "8a0aeb16cd8b73cb"),
    "tuned H128 L8 s4 FX10 FD4 in11 v1": (300352, [158464, 159744, 159872, 160064], 16, "075f7fc230524f4d"),
    "tuned H64 L4 s4 FX6 FD4 in11 v1": (42944, [22912, 23296, 23360, 23488], 0, "e022c51e63ced708"),
    "tuned H256 L8 s4 FX10 FD4 in11 v0": (955840, [492544, 495040, 495296, 496064], 16, "e2de2ba2028be441"),
}


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("mlp_pack") / "mlp_pack_dump"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "tools", "mlp_pack_dump.cpp"), "-o", str(exe)],
                   check=True)
    return json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)


def test_packer_header_is_host_only():
    """mlp_pack.h and what it includes compile without HIP: no hip header, no device qualifier."""
    text = open(os.path.join(CSRC, "mlp_pack.h")).read()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
    assert '#include "nm_internal.h"' not in text


def test_index_maps_match_the_recorded_fingerprints(dumped):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "mlp_pack_fingerprints.json")))
    assert len(want) >= 850
    assert sorted(dumped) == sorted(want)
    bad = [k for k in want if dumped[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} packed images changed, e.g. {bad[0]}: {dumped[bad[0]]} != {want[bad[0]]}"


def test_matrix_covers_the_families(dumped):
    fam = {}
    for k in dumped:
        fam.setdefault(k.split()[0], []).append(k)
    assert len(fam["tuned"]) == 3 * 2 * 4 * 3 * 2 * 3
    assert len(fam["bf16x3"]) == 12 and all("b3_fnv" in dumped[k] for k in fam["bf16x3"])
    assert len(fam["layerwise"]) == 8 and all(len(dumped[k]["linears"]) == 12 for k in fam["layerwise"])
    widths = {k.split()[1] for k in fam["generic"]}
    assert widths == {"H7", "H16", "H40", "H100", "H144", "H256", "H320", "H400", "H512"}
    assert {k.split()[4] for k in fam["generic"]} == {"FX0", "FX3", "FX10", "FX15", "FX20", "FX31"}
    assert {k.split()[5] for k in fam["generic"]} == {"FD0", "FD4", "FD16"}
    assert any(k.endswith("kch4") for k in fam["generic"]) and any(k.endswith("kch8") for k in fam["generic"])
    # single- and two-part encoding stages (more than 16 k-steps of 8: three chunks or more)
    assert any(dumped[k]["ch"][0] >= 3 for k in fam["generic"]) and any(dumped[k]["ch"][0] == 1 for k in fam["generic"])


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_tuned_anchors(dumped, name):
    n, off, skip_mask, fnv = ANCHORS[name]
    got = dumped[name]
    assert (got["n"], got["off"], got["skip_mask"], got["fnv"]) == (n, off, skip_mask, fnv)
