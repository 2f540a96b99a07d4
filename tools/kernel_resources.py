"""Register budget of the kernels of one csrc/*.hip, from the compiler's own remarks (no GPU).

    python tools/kernel_resources.py cd_rl.hip [--filter k_rl_decide] [-D FC_RL_SB=8 ...]

Compiles the file for gfx950, device side only, with the flags of fastconsensus_amd/build.py plus
-Rpass-analysis=kernel-resource-usage, and prints one line per kernel: VGPRs, SGPR spills, VGPR
spills, scratch bytes per lane, waves per SIMD, static LDS bytes per block, name (demangled where c++filt / llvm-cxxfilt is
found).  Nothing but the remarks is read: no object file is kept, no assembly is inspected.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastconsensus_amd import build as fb  # noqa: E402

FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds")]
# "file:line:col: remark: KEY: VALUE [-Rpass...]" (or "remark: file:line:col: KEY: ..." from a split compile)
REMARK = re.compile(r"remark: (?:\S+:\d+:\d+: )?\s*(.*?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]")


def remarks(src, defines=()):
    """The compiler's stderr for a device-only compile of csrc/<src> with the library's flags."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [fb.HIPCC] + fb.FLAGS + ["-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                      "-fno-caret-diagnostics"] + \
            ["-D" + d for d in defines] + ["-c", os.path.join(fb.CSRC, src), "-o", os.path.join(tmp, "dev.o")]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit("compile failed: " + " ".join(cmd))
        return p.stderr


def parse(text):
    """-> [{name, vgpr, sspill, ...}] in the order the compiler reports the kernels"""
    out = []
    for line in text.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            out.append({"name": val})
        elif out:
            for label, short in FIELDS:
                if key == label:
                    out[-1][short] = int(val)
    return out


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or \
        next((p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt",) if os.path.exists(p)), None)
    if not tool or not names:
        return names
    try:
        res = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, timeout=60)
    except (OSError, subprocess.SubprocessError):
        return names
    got = res.stdout.splitlines()
    return got if res.returncode == 0 and len(got) == len(names) else names


def short(name):
    """void fc::(anonymous namespace)::k<...>(args) -> k<...>"""
    name = re.sub(r"^void ", "", name)
    name = name.replace("fc::(anonymous namespace)::", "").replace("fc::", "")
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src", help="a file of fastconsensus_amd/csrc, e.g. cd_rl.hip")
    ap.add_argument("--filter", default="", help="only kernels whose name contains this")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra macro (an A/B switch)")
    a = ap.parse_args()
    ks = parse(remarks(a.src, a.defines))
    for k, n in zip(ks, demangle([k["name"] for k in ks])):
        k["name"] = short(n)
    print("# %s for %s%s" % (a.src, fb.ARCH, "".join(" -D" + d for d in a.defines)))
    print("# %5s %7s %7s %7s %4s %6s  %s" % ("VGPRs", "S-spill", "V-spill", "scratch", "occ", "LDS", "kernel"))
    for k in ks:
        if a.filter in k["name"]:
            print("  %5d %7d %7d %7d %4d %6d  %s" % (k.get("vgpr", -1), k.get("sspill", -1), k.get("vspill", -1),
                                                   k.get("scratch", -1), k.get("occ", -1), k.get("lds", -1), k["name"]))


if __name__ == "__main__":
    main()
