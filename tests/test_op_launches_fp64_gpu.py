"""Every non-convolution launch the passes make, against fp64, on every frame.

The ops wrappers emoportraits_amd/nets.py calls besides the convolutions -- groupnorm_affine (own reduction pass, from TileStats,
from RunSums), upsample_trilinear (plain and with gn_groups=), avgpool, add, add_rows_indexed, small_gemm, projector_finalize,
mat4_inverse, volume_to_channels_last and grid_sample3d (delta= / theta=, with and without vol_index) -- are wrapped while
the passes run eagerly at the released architecture (image_size 256: every launch of the warp generators, the 3-D U-net, the
samplers and the embedding path has its R512 per-sample shape; only the decoder's and encoder's maps shrink), default
precision, random_init checkpoints.  Each launch runs on the caller's own tensors (inputs an `out=` could overwrite are copied
first) and is compared at once, sample by sample, with the fp64 reference of tests/ops_reference.py under the bounds derived
there.  Only a summary row per launch is kept.  The convolutions have their own checker (test_conv_launches_fp64_gpu.py).

One PARITY line per pass: the worst figure per operation (call site and frame), the sampler's error ratios to ATen's fp32 CPU
kernel, and the inventory (operation, form, per-sample shape) -> launches.

The coverage guard at the end runs without a GPU: every ops.<name>( call in nets.py is wrapped here, wrapped by the conv
checker, or exempt by name with a reason.  The checker and the guard take a tuple of modules: the embedders' launches
(test_embedder_launches_fp64_gpu.py) go through the same OpLaunchChecker with their own operations registered.
"""
import inspect
import os
import re
import sys
from collections import Counter

import pytest
import torch

import ops_reference as R
from emoportraits_amd import embedders, encoder, nets, ops, stage2
from guarded_outputs import guarded_outputs  # noqa: F401  (every output ops allocates: poisoned, between guards; the GPU tests ask for it)

DEV = "cuda:0"
GRID_CAP = 8192 * 256             # work items one trip of a capped grid covers (grid_for: 8192 blocks of 256 threads)

WRAPPED = ("groupnorm_affine", "upsample_trilinear", "avgpool", "add", "add_rows_indexed", "small_gemm", "projector_finalize",
           "mat4_inverse", "volume_to_channels_last", "grid_sample3d")
CONV_CHECKER = ("conv_igemm", "conv_head")                   # test_conv_launches_fp64_gpu.LaunchChecker
EXEMPT = {"clear_overflow_flags": "a fill of the overflow words: no arithmetic; its effect is what overflow_events reads",
          "overflow_events": "a host read of the overflow words: no launch"}
_REAL, _SIG = {}, {}


def register(names):
    """keep the real ops.<name> and its signature for a wrapper to call (before anything is patched)"""
    for name in names:
        if name not in _REAL:
            _REAL[name] = getattr(ops, name)
            _SIG[name] = inspect.signature(_REAL[name])


register(WRAPPED)
NETWORK_MODULES = (nets, embedders, stage2, encoder)            # the modules whose frames name a launch's call site
_SOURCES = tuple(os.path.abspath(m.__file__) for m in NETWORK_MODULES)


def _call_site(sources=_SOURCES):
    """function:line of the innermost frame of one of the network modules that made the launch (with the block's prefix where
    the caller has one)"""
    f = sys._getframe(2)
    while f is not None and os.path.abspath(f.f_code.co_filename) not in sources:
        f = f.f_back
    if f is None:
        return "?"
    owner = f.f_locals.get("self")
    site = f"{type(owner).__name__ + '.' if owner is not None else ''}{f.f_code.co_name}:{f.f_lineno}"
    while f is not None and os.path.abspath(f.f_code.co_filename) in sources:
        prefix = getattr(f.f_locals.get("self"), "prefix", None)
        if prefix:
            return f"{prefix} {site}"
        f = f.f_back
    return site


def _overlaps(out, t):
    return isinstance(t, torch.Tensor) and ops._shares_storage(out, t)


def _before(v):
    """a copy of an argument a launch mutates, taken before the real call: a tensor, a list of tensors (the frames of a ragged
    batch) or an object that holds one as .tensor; None stays None"""
    if v is None:
        return None
    if isinstance(v, (list, tuple)):
        return type(v)(_before(t) for t in v)
    return v.clone() if isinstance(v, torch.Tensor) else type(v)(v.tensor.clone())


class OpLaunchChecker:
    """stands in for the non-conv ops attributes while a pass runs: real launch, fp64 check, one summary row"""

    wrapped = WRAPPED                     # the ops attributes this checker stands in for (a subclass names its own)
    title = "op launches"
    modules = NETWORK_MODULES             # the modules whose frames name a launch's call site
    # op -> the arguments its launch writes in place (frames, the streams' state and flags): a checker is handed their copies from
    # before the real call under their names, and the caller's own objects, as the launch left them, under "after"
    mutated = {}

    def __init__(self, tag):
        self.tag = tag
        self.rows = []
        self.intercepted = 0
        self._sources = tuple(os.path.abspath(m.__file__) for m in self.modules)
        self._inside = False              # a wrapped op that calls another one (grid_sample3d's repack): checked as the outer launch

    def install(self, mp):
        for name in self.wrapped:
            mp.setattr(ops, name, self._wrapper(name))

    def _wrapper(self, name):
        def call(*args, **kwargs):
            if self._inside:
                return _REAL[name](*args, **kwargs)
            a = _SIG[name].bind(*args, **kwargs)
            a.apply_defaults()
            a = dict(a.arguments)
            self.intercepted += 1
            site = _call_site(self._sources)
            out_arg = a.get("out")
            if out_arg is not None:       # a launch that writes into a caller's buffer: keep what it could overwrite
                a = {k: (v.clone() if _overlaps(out_arg, v) and v is not out_arg else v) for k, v in a.items()}
            if name in self.mutated:      # a launch that writes into its arguments: what they held before it
                a["after"] = {k: a[k] for k in self.mutated[name]}
                a.update({k: _before(a[k]) for k in self.mutated[name]})
            self._inside = True
            try:
                result = _REAL[name](*args, **kwargs)
                form, shape, fig = getattr(self, "_check_" + name)(a, result)
            finally:
                self._inside = False
            # (a launch whose result does not carry its rows -- frames pasted into in place, a bank -- says their number itself)
            batch = fig["batch"] if "batch" in fig else (result[0] if isinstance(result, tuple) else result).shape[0]
            self.rows.append(dict(op=name, form=form, shape=shape, site=site, batch=batch, frames=len(fig["frames"]),
                                  worst=fig["worst"], frame=fig["worst_frame"], unit=fig["unit"], failures=fig["failures"],
                                  max_ratio=fig.get("max_ratio"), mean_ratio=fig.get("mean_ratio"), yardstick=fig.get("yardstick"),
                                  rms=fig.get("rms_rel"), extra=fig.get("extra")))
            return result
        return call

    # ---- one checker per operation: (arguments, result) -> (form, per-sample shape, figures) -----------------------------
    def _check_volume_to_channels_last(self, a, out):
        return "", tuple(a["vol"].shape[1:]), R.check_channels_last(out, a["vol"])

    def _check_add(self, a, out):
        return f"period {a['b'].numel()}", tuple(a["a"].shape[1:]), R.check_add(out, a["a"], a["b"], a["alpha"])

    def _check_add_rows_indexed(self, a, out):
        return f"K={a['table'].shape[0]}", tuple(a["a"].shape[1:]), R.check_add_rows_indexed(out, a["a"], a["table"], a["index"], a["alpha"])

    def _check_avgpool(self, a, out):
        return tuple(a["kernel"]), tuple(a["x"].shape[1:]), R.check_avgpool(out, a["x"], a["kernel"])

    def _check_upsample_trilinear(self, a, result):
        out, sums = result if a["gn_groups"] is not None else (result, None)
        if sums is not None:              # the sums are checked where groupnorm_affine consumes them: against x's own statistics
            assert sums.shape == tuple(out.shape) and 1 <= sums.split <= 64, (sums.shape, sums.split)
        form = (tuple(a["factors"]), "sums" if sums is not None else "plain")
        return form, tuple(a["x"].shape[1:]), R.check_upsample_trilinear(out, a["x"], a["factors"])

    def _check_groupnorm_affine(self, a, result):
        scale, shift = result[:2]
        st = a["stats"]
        form = "sums" if isinstance(st, ops.RunSums) else "tiles" if st is not None else "pass"
        if a["ada_gamma"] is not None:
            form += "+ada"
        fig = R.check_groupnorm_affine(scale, shift, a["x"], a["gamma"], a["beta"], a["ada_gamma"], a["ada_beta"], a["groups"], a["eps"])
        return form, tuple(a["x"].shape[1:]), fig

    def _check_small_gemm(self, a, out):
        return f"NN={a['NN']}", tuple(a["A"].shape), R.check_small_gemm(out, a["A"], a["B"], a["NN"])

    def _check_projector_finalize(self, a, result):
        fig = R.check_projector_finalize(result[0], result[1], a["T"], a["V"], a["norm_of_row"], a["gamma"], a["beta"])
        return "", tuple(a["T"].shape[1:]), fig

    def _check_mat4_inverse(self, a, out):
        return "", (4, 4), R.check_mat4_inverse(out, a["m"])

    def _check_grid_sample3d(self, a, out):
        if a["grid"] is not None or a["in_layout"] == "p4" or a["out_layout"] == "p4":
            raise AssertionError("a sampler form the passes did not use when this checker was written: give it a reference")
        kind = "delta" if a["delta"] is not None else "theta"
        form = f"{kind} {a['in_layout']}->{a['out_layout']}" + (" indexed" if a["vol_index"] is not None else "")
        fig = R.check_grid_sample3d(out, a["vol"], a["delta"], a["theta"], a["padding_mode"], a["in_layout"], a["out_layout"],
                                    a["vol_index"])
        return form, tuple(a["vol"].shape[1:]), fig

    # ---- after the pass --------------------------------------------------------------------------------------------------
    def inventory(self):
        return Counter((r["op"], r["form"], r["shape"]) for r in self.rows)

    def has(self, op, form=None, shape=None):
        return [r for r in self.rows if r["op"] == op and (form is None or (form(r["form"]) if callable(form) else r["form"] == form))
                and (shape is None or shape(r["shape"]))]

    def report(self):
        assert self.rows, f"{self.tag}: no launch was intercepted"
        parts = []
        for name in self.wrapped:
            rows = [r for r in self.rows if r["op"] == name]
            if not rows:
                continue
            w = max(rows, key=lambda r: r["worst"])
            s = f"{name} {w['worst']:.3g} {w['unit']} ({w['form']} {w['site']}, frame {w['frame']})"
            held = [r for r in rows if r["max_ratio"] is not None]
            if held:                                       # held to a yardstick (the samplers)
                s += (f"; error ratios to {held[0]['yardstick']}: " + ", ".join(
                    f"{r['form']} max {r['max_ratio']:.3f} mean {r['mean_ratio']:.3f}" for r in _worst_per_form(held)))
            if rows[0]["rms"] is not None:
                rms = sorted(r["rms"] for r in rows)
                s += f"; rms err / rms ref: worst {rms[-1]:.2e}, median {rms[len(rms) // 2]:.2e}"
                by_form = {}
                for r in rows:
                    by_form[r["form"]] = max(by_form.get(r["form"], 0.0), r["rms"])
                s += ", worst per form: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(by_form.items()))
            parts.append(s)
        inv = self.inventory()
        print(f"PARITY {self.title} vs fp64 [{self.tag}]: {len(self.rows)} launches; worst per operation: " + "; ".join(parts)
              + "; inventory (operation, form, per-sample shape) -> launches: " + str(dict(sorted(inv.items(), key=str))))
        return inv

    def assert_clean(self):
        bad = [f"{r['op']} {r['form']} {r['shape']} at {r['site']}: {f}" for r in self.rows for f in r["failures"]]
        assert not bad, f"{self.tag}: {len(bad)} violations:\n" + "\n".join(bad[:40])
        assert len(self.rows) == self.intercepted, "an intercepted launch has no row"
        short = [(r["op"], r["site"], r["frames"], r["batch"]) for r in self.rows if r["frames"] != r["batch"]]
        assert not short, f"launches not checked on every frame: {short}"


def _worst_per_form(rows):
    best = {}
    for r in rows:
        if r["form"] not in best or r["max_ratio"] > best[r["form"]]["max_ratio"]:
            best[r["form"]] = r
    return [best[k] for k in sorted(best)]


def _run(monkeypatch, tag, fn):
    chk = OpLaunchChecker(tag)
    with monkeypatch.context() as mp:
        chk.install(mp)
        fn()
    torch.cuda.synchronize()
    inv = chk.report()
    chk.assert_clean()
    return chk, inv


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _driver_pass(B, seed, bank=None):
    from test_nets_gpu import _full_size
    cfg, sd, x = _full_size(256, B, seed=seed)
    hp = nets.HotPath(sd, cfg, DEV, with_source=False)
    d = lambda t: t.to(DEV)
    canon, idt = [x["canonical"]], [x["idt"]]
    if bank:
        g = torch.Generator().manual_seed(seed + 7)
        canon.append((0.8 * x["canonical"].flip(-1) + 0.05 * torch.randn(x["canonical"].shape, generator=g)).contiguous())
        idt.append((x["idt"] + 0.3 * torch.randn(x["idt"].shape, generator=g)).contiguous())
    ccl = torch.cat([hp.prepare_canonical(d(c)) for c in canon])
    identity = torch.tensor(bank, dtype=torch.int32, device=DEV) if bank else None
    return hp, lambda: hp.driver_pass(ccl, d(torch.cat(idt)), d(x["pose_t"]), d(x["th_t"]), identity=identity)


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
def test_driver_pass_every_op_launch_vs_fp64(monkeypatch):
    """B = 5, the smallest batch at which a capped grid (grid_for: 8192 blocks) actually loops: the depth pooling (2, 1, 1) of the
    warp generator's last block writes B x 32 x 16 x 64 x 64 outputs, four per thread of avgpool_x4_kernel -- B x 524288 quads
    against the 8192 x 256 = 2097152 one trip covers: B = 4 fills the grid exactly, B = 5 is the first with a second trip."""
    B = 5
    hp, fn = _driver_pass(B, seed=256)
    chk, inv = _run(monkeypatch, f"driver R256 B={B}", fn)
    pools = chk.has("avgpool", (2, 1, 1))
    assert pools, inv
    quads = max(B * _numel(r["shape"]) // 2 // 4 for r in pools)
    assert quads > GRID_CAP and (B - 1) * quads // B <= GRID_CAP, (quads, GRID_CAP)       # loops at B, would not at B - 1
    for form in ("pass", "tiles", "sums"):
        assert chk.has("groupnorm_affine", lambda f: f.split("+")[0] == form), (form, inv)
    assert chk.has("groupnorm_affine", lambda f: f.endswith("+ada")), inv
    assert chk.has("upsample_trilinear", lambda f: f[1] == "sums"), inv
    assert chk.has("small_gemm", "NN=1") and chk.has("small_gemm", "NN=16"), inv
    assert chk.has("projector_finalize") and chk.has("add"), inv
    assert chk.has("grid_sample3d", "delta ndhwc->ndhwc") and chk.has("grid_sample3d", "theta ndhwc->ncdhw"), inv
    assert all(r["shape"] == (16, 64, 64, 96) for r in chk.has("grid_sample3d")), inv    # the released latent volume
    assert not chk.has("add_rows_indexed"), inv


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
def test_driver_pass_with_identity_bank_every_op_launch_vs_fp64(monkeypatch):
    """K = 2 identities, B = 3 frames, identity = [1, 0, 1]: the indexed add and the indexed uv sampler read the bank"""
    hp, fn = _driver_pass(3, seed=257, bank=[1, 0, 1])
    chk, inv = _run(monkeypatch, "driver R256 B=3 bank K=2", fn)
    rows = chk.has("add_rows_indexed")
    assert rows and all(r["frames"] == 3 and r["form"] == "K=2" for r in rows), inv
    rows = chk.has("grid_sample3d", "delta ndhwc->ndhwc indexed")
    assert rows and sum(r["frames"] for r in rows) == 3, inv
    assert not chk.has("add") and not chk.has("grid_sample3d", "delta ndhwc->ndhwc"), inv


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
def test_source_pass_every_op_launch_vs_fp64(monkeypatch):
    from test_nets_gpu import _full_size
    cfg, sd, x = _full_size(256, 1, seed=21)
    hp = nets.HotPath(sd, cfg, DEV)
    d = lambda t: t.to(DEV)
    chk, inv = _run(monkeypatch, "source R256 B=1",
                    lambda: hp.source_pass(d(x["img"]), d(x["idt"]), d(x["pose_s"]), d(x["th_s"])))
    plain = lambda fac: chk.has("upsample_trilinear", (fac, "plain"))
    assert plain((2, 1, 1)) and plain((2, 2, 2)) and plain((1, 2, 2)), inv                # (2, 1, 1): the one-output-per-thread kernel
    assert chk.has("avgpool", lambda f: len(f) == 2), inv
    for k in ((2, 2, 2), (1, 2, 2), (2, 1, 1)):
        assert chk.has("avgpool", k), (k, inv)
    assert chk.has("add", shape=lambda s: _numel(s) > GRID_CAP), inv                      # add_kernel's grid-stride loop runs twice
    assert chk.has("mat4_inverse") and chk.has("volume_to_channels_last"), inv
    assert chk.has("grid_sample3d", "theta ndhwc->ndhwc") and chk.has("grid_sample3d", "delta ndhwc->ncdhw"), inv
    for form in ("pass", "tiles", "sums"):
        assert chk.has("groupnorm_affine", lambda f: f.split("+")[0] == form), (form, inv)


def ops_called(*modules):
    """the names of every ops.<name>( call in the source of the given modules"""
    called = set()
    for m in modules:
        with open(os.path.abspath(m.__file__)) as f:
            called |= set(re.findall(r"\bops\.(\w+)\(", f.read()))
    return called


def test_every_ops_call_of_the_networks_is_checked_or_exempt():
    """a launch added to the passes later cannot go unchecked without someone deciding so"""
    called = ops_called(nets)
    assert {"conv_igemm", "groupnorm_affine", "grid_sample3d"} <= called, called            # (the pattern still finds the calls)
    unchecked = sorted(called - set(WRAPPED) - set(CONV_CHECKER) - set(EXEMPT))
    assert not unchecked, f"ops called by nets.py that no launch checker wraps: {unchecked}"
    assert all(hasattr(OpLaunchChecker, "_check_" + name) and callable(getattr(ops, name)) for name in WRAPPED)
    from test_conv_launches_fp64_gpu import LaunchChecker
    assert all(callable(getattr(LaunchChecker, name, None)) for name in CONV_CHECKER)
    assert all(reason for reason in EXEMPT.values())
