"""CPU test: emo_conv_accepts (ABI 24) answers for every convolution entry without a device.

A child process loads the product library with ctypes -- no torch, no other call into it -- and asks once for a launch the entry
takes and once for one it refuses, with the CU count given.  The codes are the entries' own (a misaligned output of the phase form
is EMO_ERR_ALIGN, not EMO_ERR_UNSUPPORTED), the fill rule of the pair kernels follows the CU count that is passed, and the child
holds the same device files open after the questions as before them: none, on a machine that has them too."""
import json
import os
import subprocess
import sys

from emoportraits_amd import hip, pack

CHILD = r"""
import ctypes, json, os, sys
lib = ctypes.CDLL(sys.argv[1])
lib.emo_conv_accepts.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)] + [ctypes.c_int] * 15 + [ctypes.c_float] * 2 + [ctypes.c_int]
def devices():
    fds = []
    for fd in os.listdir("/proc/self/fd"):
        try:
            fds.append(os.readlink("/proc/self/fd/" + fd))
        except OSError:
            pass
    return sorted(p for p in fds if p.startswith(("/dev/kfd", "/dev/dri")))
before, codes = devices(), []
for entry, tensors, ints, ncu in json.load(sys.stdin):
    codes.append(lib.emo_conv_accepts(entry, (ctypes.c_int * 12)(*tensors), *ints, 32.0, 1.0, ncu))
print(json.dumps({"codes": codes, "opened": [p for p in devices() if p not in before]}))
"""


def _question(entry, cout=64, cin=8, H=8, W=64, N=1, taps=(1, 3, 3), ups=0, cfg=pack.CFG_D, ncu=256, **tensors):
    """(entry, tensors, N .. ksplit, ncu): an aligned launch without affine, residual or K split unless `tensors` says otherwise"""
    t = dict(x=0, wpk=0, wpk16=0 if entry == "f16w8_rest" else -1, bias=-1, scale=-1, shift=-1, res=-1, out=0, workspace=-1, gn_stats=-1,
             flag=-1, run_if=0 if entry == "f32_guarded" else -1)
    t.update(tensors)
    return [pack._ENTRIES[entry], list(t.values()), [N, cin, cout, 1, H, W, *taps, ups, 0, 0, 0, cfg, 1], ncu]


#          the entry takes it                                       ... and refuses it, with the code of the condition that is missed
CASES = [(_question("f32", cfg=pack.CFG_B),                         _question("f32", cfg=pack.CFG_B, W=48), -2),
         (_question("f32_guarded", cfg=pack.CFG_B),                 _question("f32_guarded", cfg=pack.CFG_B, x=-1), -1),
         (_question("bf16x3"),                                      _question("bf16x3", cin=12), -2),
         (_question("f16x2"),                                       _question("f16x2", x=4), -2),
         (_question("f16x2", H=2, ups=1, cfg=pack.CFG_F16X2_UP2),   _question("f16x2", H=2, ups=1, cfg=pack.CFG_F16X2_UP2, out=8), -3),
         (_question("f16"),                                         _question("f16", cin=1032, scale=0, shift=0), -2),
         (_question("f16w8", cout=128, H=512, W=512),               _question("f16w8", cout=128, H=64), -2),
         (_question("f16w8", cout=128, H=64, ncu=8),                _question("f16w8", cout=128, H=64, ncu=16), -2),
         (_question("f16w8_rest", cout=192, H=512, W=512),          _question("f16w8_rest", cout=128, H=512, W=512), -2)]


def test_every_entry_answers_without_a_device():
    assert {q[0] for case in CASES for q in case[:2]} == set(pack._ENTRIES.values())
    env = {k: v for k, v in os.environ.items() if not k.startswith(("EMO_", "HIP_VISIBLE", "ROCR_VISIBLE"))}
    r = subprocess.run([sys.executable, "-c", CHILD, hip.LIB_PATH], input=json.dumps([q for case in CASES for q in case[:2]]),
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert got["opened"] == [], "a question opened a device"
    assert got["codes"] == [code for case in CASES for code in (0, case[2])]


def test_the_planner_s_question_is_the_library_s():
    """pack.launch_accepted on its own: the decoder's 512 -> 320 up-convolution at 16 frames in the phase form, and not with a residual"""
    up = dict(cout=320, cin=512, kd=1, kh=3, kw=3, N=16, D=1, H=64, W=64, ups=True, cfg=pack.CFG_F16X2_UP2)
    assert pack.launch_accepted("f16x2", **up) and not pack.launch_accepted("f16x2", res=True, **up)
    assert pack.up2_launch_fits(320, 512, 1, 3, 3, 16, 64, 64, True) == pack.up2_enabled()
