"""TEST INFRASTRUCTURE ONLY -- the facade the emulated tests put in front of the host-compiled library (tests/emul/emulibs.py) so
that emoportraits_amd.ops runs on CPU tensors: every entry point gets the argument and result types of emoportraits_amd.hip, and
every call is counted under its entry's name and written down in call order.  The ABI 22 crop and paste serve the one-window-per-frame form and the
several-faces-per-frame form under ONE name (`frame_of` null or not), so for those two the form of every call is recorded too."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emo_hip.h")
TWO_FORMS = ("emo_yuv420_crop_f32", "emo_paste_yuv420")


def argument_index(name, argument):
    """(the position of `argument` in the prototype of `name` in include/emo_hip.h, the number of its parameters)"""
    proto = re.search(r"\bint %s\(([^)]*)\)" % re.escape(name), open(HEADER).read())
    params = [p.split()[-1].lstrip("*") for p in proto.group(1).split(",")]
    return params.index(argument), len(params)


class _Calls(dict):
    """{entry name: calls}; .forms = {name of a TWO_FORMS entry: ['windows' | 'faces' per call, in call order]}; .order = the entry
    names of all calls in call order; clear() empties all three"""

    def __init__(self):
        super().__init__()
        self.forms, self.order = {}, []

    def clear(self):
        super().clear()
        self.forms.clear()
        self.order.clear()


class CountingLib:
    """the host-compiled stream library behind emoportraits_amd.hip's table of signatures; .calls counts the calls, .forms is
    .calls.forms, .order is .calls.order"""

    def __init__(self, lib):
        from emoportraits_amd import hip
        self._lib, self._sig, self._res, self.calls = lib, hip.SIGNATURES, hip._RESTYPES, _Calls()
        self._frame_of = {}
        for name in TWO_FORMS:
            at, n = argument_index(name, "frame_of")
            assert n == len(self._sig[name]), f"{name}: the header has {n} parameters, hip.SIGNATURES {len(self._sig[name])}"
            self._frame_of[name] = at

    @property
    def forms(self):
        return self.calls.forms

    @property
    def order(self):
        return self.calls.order

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        fn = getattr(self._lib, name)
        fn.argtypes, fn.restype = self._sig[name], self._res.get(name, ctypes.c_int)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            self.calls.order.append(name)
            if name in self._frame_of:
                self.forms.setdefault(name, []).append("windows" if args[self._frame_of[name]] is None else "faces")
            return fn(*args)
        return counted
