"""sha256 of the gfx950 device assembly of the convolution units (conv_api.hip, conv_inst_*.hip), to hold a host-side change to
"the device code is the same": compiled with the flags of emoportraits_amd/build.py plus --cuda-device-only -S.

    python tools/device_code_digest.py [CSRC_DIR] [-DNAME=V ...] > digests.json
                                                                       {unit: digest}, CSRC_DIR: another checkout's csrc; -DNAME=V:
                                                                       a measurement build (as tools/kernel_resources.py --audit)
    python tools/device_code_digest.py --diff A.json B.json            the units whose digests differ (exit status 1 if any)

The digest covers every line of the assembly -- instruction streams, kernel descriptors, metadata -- except what names the source
file and not its code: the .file directives, and the hash in the unit's one-byte __hip_cuid_<hash> symbol (hipcc derives it from
the path and text of the source)."""
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emoportraits_amd import build  # noqa: E402


def digest(src):
    cmd = [build.HIPCC] + build.FLAGS + build.EXTRA_FLAGS.get(os.path.basename(src), []) + ["--cuda-device-only", "-S", src, "-o", "-"]
    asm = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in asm.splitlines() if not ln.lstrip().startswith(".file")]
    return hashlib.sha256(re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", "\n".join(lines)).encode()).hexdigest(), len(lines)


def main(argv):
    if argv[:1] == ["--diff"]:
        a, b = (json.load(open(p)) for p in argv[1:3])
        bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        print("identical" if not bad else "DIFFERENT: " + ", ".join(bad))
        return 1 if bad else 0
    while argv and argv[-1].startswith("-D"):
        build.FLAGS = build.FLAGS + [argv.pop()]
    csrc = argv[0] if argv else build.CSRC
    units = sorted(f for f in os.listdir(csrc) if f == "conv_api.hip" or (f.startswith("conv_inst_") and f.endswith(".hip")))
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        res = list(ex.map(lambda f: digest(os.path.join(csrc, f)), units))
    json.dump({f: {"sha256": d, "lines": n} for f, (d, n) in zip(units, res)}, sys.stdout, indent=1)
    print()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
