"""Static resource table of every gfx950 kernel in the product library: VGPRs, SGPRs, scratch bytes, static LDS,
register spills, the launch bound and a digest of the instruction stream -- read from the compiler's assembly, no GPU needed.

    python scripts/kernel_resources.py [source.hip ...] [> profiles/rNN_kernel_resources.txt]

Each .hip source is compiled device-only with the product flags (nerfmeshes_amd/build.py) to assembly; the AMDGPU metadata
and the kernel bodies are parsed from the text.  What to look for: `scr` must be 0 for every fp32 MLP kernel (scratch stores
go through to HBM), `v` decides waves per SIMD (512 / v, at most 8).

`digest` answers "did this refactor change the code the GPU runs?": a hash over the kernel's instructions and its
.amdhsa register / LDS / scratch sizes, with everything that only names things taken out (comments, mangled names -- they
change when a template parameter disappears --, the function index in block labels).  Two trees compile to the same kernels
exactly when, per source, the sorted digest columns are equal:

    python scripts/kernel_resources.py | awk 'NR > 1 {print $1, $9}' | sort     # diff this between the two trees
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfmeshes_amd import build as B  # noqa: E402

FIELDS = (("v", "vgpr_count"), ("s", "sgpr_count"), ("scr", "private_segment_fixed_size"),
          ("lds", "group_segment_fixed_size"), ("spill_v", "vgpr_spill_count"), ("spill_s", "sgpr_spill_count"),
          ("wg", "max_flat_workgroup_size"))
AMDHSA = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def digest_of(asm, symbol):
    """Hash of one kernel: its instruction lines (labels included) and the AMDHSA values, names normalised away."""
    body = asm[asm.index(f"\n{symbol}:") + 1:]
    body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
    desc = re.search(r"\.amdhsa_kernel " + re.escape(symbol) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
    lines = [re.sub(r"\s+", " ", line.split(";")[0]).strip() for line in body.splitlines()[1:]]
    lines = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "_Z", line)) for line in lines if line]
    lines += [re.search(r"\.amdhsa_" + key + r"\s+\S+", desc).group(0) for key in AMDHSA]
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], len(lines) - len(AMDHSA)


def kernels_of(src, tmp):
    out = os.path.join(tmp, os.path.splitext(src)[0] + ".s")
    subprocess.run([B.hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", out], check=True)
    asm = open(out).read()
    rows = []
    for block in re.split(r"\n\s+- \.agpr_count:", asm[asm.index(".amdgpu_metadata"):])[1:]:
        def field(key):
            m = re.search(r"\." + key + r":\s+(\S+)", block)
            return m.group(1) if m else "?"
        digest, instructions = digest_of(asm, field("name"))
        name = subprocess.run(["c++filt", field("name")], capture_output=True, text=True).stdout.strip()
        rows.append((re.sub(r"^void ", "", re.sub(r"\(.*", "", name)), [field(k) for _, k in FIELDS] + [digest], instructions))
    return rows


def main():
    only = sys.argv[1:]
    sources = [s for s in B.SOURCES if s.endswith(".hip") and (not only or s in only)]
    print(f"{'source':16s} " + " ".join(f"{h:>7s}" for h, _ in FIELDS) + f" {'digest':>16s}  kernel")
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(int(os.environ.get("NM_BUILD_JOBS", "0")) or os.cpu_count() or 4) as pool:
        for src, rows in zip(sources, pool.map(lambda s: kernels_of(s, tmp), sources)):
            for name, vals, _ in sorted(rows):
                print(f"{src:16s} " + " ".join(f"{v:>7s}" for v in vals[:-1]) + f" {vals[-1]:>16s}  " + name)
            print(f"# {src}: {len(rows)} kernels, {sum(r[2] for r in rows)} instruction lines", file=sys.stderr)


if __name__ == "__main__":
    main()
