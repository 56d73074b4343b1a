"""Drop-in `InferenceWrapper` for the MI355X hot path -- SURVEY.md section 8(b), seams b1 (user API) and b2 (model attributes).

Mirrors notebooks/infer.py of the reference: same constructor and `forward` signature (infer.py:63-65, :355-357),
same files (`<project_dir>/<folder>/<experiment_name>/args.txt`, `.../checkpoints/<model_file_name>`), same cached
attributes after a source call (`idt_embed`, `source_latent_volume`, `target_latent_volume`, `pred_source_theta`, ...)
and the same return value `(List[PIL.Image], Tensor[B,3,S,S])` / `None`.

The embedders that feed the hot path -- IdtEmbed (ResNet-50), ExpressionEmbed and HeadPoseRegressor (ResNet-18s), SURVEY.md
section 8f-1 -- run on the HIP kernels too (emoportraits_amd/embedders.py): they are built from the `idt_embedder_nw.*` /
`expression_embedder_nw.*` keys of the checkpoint and from `head_pose_regressor_path` (args.txt or constructor argument,
va_arguments.py:26) whenever those are present.

What is NOT here, by scope: the third-party nets outside the checkpoint -- face detector / cropper (mediapipe), face
parsing (BiSeNet), matting (MODNet).  They plug in through `embedders=` (any callables; an entry there also overrides a
native embedder); without them `forward` needs `crop=False` and `source_mask=`.  Embeddings can also be supplied directly
through the reference's own hooks `custome_target_pose_embed` / `custome_target_theta_embed` (infer.py:565-566,603-604)
and their source-side counterparts added here (`custome_source_pose_embed`, `custome_source_theta_embed`,
`custome_idt_embed`).  Missing pieces raise -- nothing falls back silently.

Extension over the reference (which is batch-1, F5): driver inputs may carry a batch dimension, and
`animate()` streams N driver frames in device-sized batches, sharded across ranks (emoportraits_amd/parallel.py).
With `identity_capacity=K` the wrapper also keeps a bank of K source identities on the device (`store_identity`,
`load_identity`, `drop_identity`, `identities`, `share_identity`; `enrol_identities` fills it K sources at a time, sharded across
ranks), and `animate` / `animate_frames(identities=...)` render
frames of several identities in one driver batch.  Both batched entry points take forward()'s pose controls -- `mix` / `mix_old`
(get_mixing_theta), `target_theta` and `smooth_pose` -- on the device (ops.mixing_theta, ops.theta_ema_scan, a gather of the
source thetas): with a bank, every frame is mixed against its own identity's source theta, and with smooth_per_identity=True
smoothed within its own identity's frame sequence (one EMA stream per slot, reset by store / drop / reset_pose_state).
"""
import functools
import os
import pathlib
from argparse import Namespace

import torch

from . import config as cfg_mod
from . import embedders as emb_mod
from . import frames as frames_mod
from . import control_streams, graphs, hostglue, nets, ops, parallel, schema


# smooth_pose in animate_frames: the crops of a rank's shard stay resident between the head-pose pass and the render pass up to
# this many bytes (3 MB per 512^2 frame; beyond it they are cropped a second time)
_SMOOTH_KEEP_BYTES = int(float(os.environ.get("EMO_SMOOTH_KEEP_GB", "16")) * (1 << 30))


def _sequence(key):
    """A per-frame launch sequence of the wrapper, written once: the decorated method is the eager path, and with use_graphs
    the same method is what graphs.Graphed captures under `_graphed[key]` (InferenceWrapper._capture) and the call replays"""
    def wrap(fn):
        @functools.wraps(fn)
        def call(self, *tensors):
            g = self._graphed.get(key)
            return fn(self, *tensors) if g is None else g(*tensors)
        call.key, call.eager = key, fn
        return call
    return wrap


class HipModel:
    """The `self.model` attribute seam (b2): reference attribute names and call signatures over the HIP executors."""

    def __init__(self, hot_path, args):
        self.hp = hot_path
        self.args = args
        c = hot_path.cfg
        d, s = c["latent_volume_depth"], c["latent_volume_size"]
        gs, gz = torch.linspace(-1, 1, s), torch.linspace(-1, 1, d)
        w, v, u = torch.meshgrid(gz, gs, gs, indexing="ij")
        # models/stage_1/volumetric_avatar/va.py:101-105
        self.identity_grid_3d = torch.stack([u, v, w, torch.ones_like(u)], dim=3).view(1, -1, 4).to(hot_path.device)
        self._ident3 = torch.stack([u, v, w], 0)[None].contiguous().to(hot_path.device)   # [1,3,d,s,s]
        self.embed_size = c["gen_embed_size"]
        self.resize_warp_func = lambda x: x        # warp_output_size == gen_latent_texture_size is enforced by config

    # va.py:264-265
    def grid_sample(self, inputs, grid):
        return ops.grid_sample3d(inputs.float().contiguous(), grid.float().contiguous(),
                                 padding_mode=self.hp.pad)

    def local_encoder_nw(self, img):
        return self.hp.local_encoder(img.float().contiguous())

    def volume_source_nw(self, vol):
        return self.hp.volume_source(vol.contiguous())

    def volume_process_nw(self, vol, embed_dict=None):
        return self.hp.volume_process(vol.contiguous())

    def _warp_from_delta(self, delta):
        # warp_generator_resnet.py:178: (identity_grid + deltas).permute(0, 2, 3, 4, 1) -- a permuted view, as there
        return ops.add(delta, self._ident3.reshape(-1)).permute(0, 2, 3, 4, 1)

    def xy_generator_nw(self, embed_dict):
        delta = self.hp.xy_generator(embed_dict["orig"].contiguous())
        return [self._warp_from_delta(delta), delta]

    def uv_generator_nw(self, embed_dict):
        delta = self.hp.uv_generator(embed_dict["orig"].contiguous())
        return [self._warp_from_delta(delta), delta]

    def decoder_nw(self, data_dict, embed_dict, feat_2d, input_flip_feat=False, stage_two=False, **_):
        img, feat, img_f = self.hp.decoder(feat_2d.contiguous())
        if stage_two:
            return img, None, feat, img_f
        return img, None, None, None

    def predict_embed(self, data_dict):
        """va.py:813-885 -> (source, target, mixing, embed_dict); the mixing branch is a training construct (None)."""
        idt = data_dict["idt_embed"]
        out = []
        for key in ("source_pose_embed", "target_pose_embed"):
            e = self.hp.embed(data_dict[key].float().contiguous(), idt.float().contiguous())
            out.append({"orig": e, "orig_d": e, "ada_v": data_dict[key]})
        return out[0], out[1], None, {}


class InferenceWrapper:
    def __init__(self, experiment_name, which_epoch='latest', model_file_name='', use_gpu=True, num_gpus=1,
                 fixed_bounding_box=False, project_dir='./', folder='mp_logs', model_='va',
                 torch_home='', debug=False, print_model=False, print_params=True, args_overwrite={}, state_dict=None,
                 pose_momentum=0.5, rank=0, args_path=None, embedders=None, head_pose_regressor_path=None,
                 use_graphs=True, precision=None, identity_capacity=0):
        if not use_gpu:
            raise RuntimeError("emoportraits_amd runs on MI355X only: use_gpu=False is not supported (no CPU path)")
        if model_ != 'va':
            raise ValueError("only the stage-1 'va' model is on the MI355X hot path")
        self.use_gpu, self.debug, self.num_gpus = use_gpu, debug, num_gpus
        args_path = pathlib.Path(project_dir) / folder / experiment_name / 'args.txt' if args_path is None else args_path
        found = cfg_mod.parse_args_txt(args_path)                                  # infer.py:74-76
        found['project_dir'] = project_dir
        for k, v in (args_overwrite or {}).items():                                # infer.py:79-81
            found[k] = v
        self.args = Namespace(**found)
        self.cfg = cfg_mod.hot_path_config(found, released=False) if 'norm_layer_type' in found else \
            cfg_mod.hot_path_config(found)
        for k, v in self.cfg.items():
            setattr(self.args, k, v)
        if torch_home:
            os.environ['TORCH_HOME'] = torch_home
        # one process per GPU (infer.py:94-105 uses the same env:// rendezvous)
        if num_gpus > 8:
            raise RuntimeError("at most 8 GPUs per node")                          # infer.py:104-105 (bare raise there)
        if num_gpus > 1:
            self.rank, self.world = parallel.init_distributed()
        else:
            self.rank, self.world = 0, 1
        self.device = torch.device("cuda", parallel.local_device_index())
        torch.cuda.set_device(self.device)
        self._init_state(use_graphs, int(identity_capacity), pose_momentum, fixed_bounding_box, bool(found.get('use_seg', False)))

        self.model_checkpoint = pathlib.Path(project_dir) / folder / experiment_name / 'checkpoints' / model_file_name
        self.model_dict = torch.load(self.model_checkpoint, map_location='cpu') if state_dict is None else state_dict
        schema.check_state_dict(self.model_dict, self.cfg)        # strict: the reference's strict=False hides mismatches
        self.hot_path = nets.HotPath(self.model_dict, self.cfg, self.device, precision=precision)   # 'f16': opt-in, see nets.HotPath
        self.model = HipModel(self.hot_path, self.args)
        if rank == 0 and print_params:
            n = sum(v.numel() for k, v in self.model_dict.items() if k.startswith(schema.HOT_PATH_PREFIXES))
            print(f'Number of hot-path parameters: {n}')
        native = self._native_embedders(found, head_pose_regressor_path)
        self.embedders = {**native, **dict(embedders or {})}
        # hipGraph replay of the per-frame sequences (emoportraits_amd/graphs.py); only this repo's own executors are
        # captured, user-supplied embedder callables always run eagerly
        # On by default: a drop-in user calls forward() one frame at a time, which is launch-bound without the replay
        # (bench.py extras: emotion_driver_forward_fps, latency_b1_ms).  The first call of an input signature runs eagerly,
        # the second captures, later ones replay (use_graphs='eager_first' semantics; use_graphs=False never captures).
        cls = type(self)
        self._capture(cls._drive)
        if self.identity_capacity > 0:
            self._capture(cls._drive_bank)
        for seq in (cls._head_pose, cls._expression_pass):
            if native.get(seq.key) is not None and self.embedders[seq.key] is native[seq.key]:
                self._capture(seq)

    def _init_state(self, use_graphs=True, identity_capacity=0, pose_momentum=0.5, fixed_bounding_box=False, use_seg=False):
        """Every attribute the methods read that is not a model, from the constructor's arguments alone (the identity bank
        also reads `cfg` and `device`, which must be set): crop tracking, the smooth_pose state, the per-identity cache, the
        captured graphs, the attached stage 2, the bank.  __init__ calls it before it builds the models; a test rig calls it on
        a bare object."""
        self.use_graphs = bool(use_graphs)
        self._graph_eager_calls = 0 if use_graphs == 'capture_first' else 1
        self._graphed = {}
        self.fixed_bounding_box = fixed_bounding_box
        self.momentum = 0.01
        self.center = self.size = self._crop_tracker = None
        self.pose_momentum = pose_momentum
        # the one stream of the current identity (smooth_pose's EMA, which `theta` reads; the controls' anchors and EMA), walked by
        # the calls without identities=; the bank's streams, one per slot, are _init_identity_bank's
        self._stream = control_streams.StreamStates(1, self.device, "the current identity's stream")
        self.norm_momentum = 0.1
        self.delta_yaw = self.delta_pitch = None
        self.resize_warp = False
        self.use_seg = use_seg
        self.target_latent_volume = self._canonical_cl = self.idt_embed = self.pred_source_theta = None
        # the current identity's source expression (the expression controls' neutral) and its source (scale, rotation, translation)
        # as one [1,9] row (the head-pose controls' source pose; None where the source theta came as a 4x4 matrix)
        self.pred_source_pose_embed = self.pred_source_srt = None
        self._stage2 = self._stage2_wrapper = None                                 # attach_stage2()
        # crop tracking of animate_frames(boxes=): the tracks' state on the device (control_streams.CropStates, made at the first
        # use), apart from the host _crop_tracker of forward(crop=True); tracked_windows = (the paste windows of the chunk last
        # tracked, int32 [rows,4] on the device, side 0 = no face; the index of its first row in the call).  detections=: the
        # tracks the detections are associated to (control_streams.TrackStates), and tracked_assignment = (track_of [n,D], restart
        # [n,P]) of the chunk last tracked, int32 on the device.  tracking follow_tracks=True: tracked_present = (present int32 [rows]
        # on the device: 1 where the row has a face, the index of its first row), beside tracked_windows.  tracking skip_absent=True:
        # tracked_rows = (row_of int32 [T] on the device: the row of the chunk that each rendered row is, first: the rendered rows
        # in front of every frame of the chunk, a host list of n + 1, the index of the chunk's first row in the call)
        self._crop_streams = self.tracked_windows = None
        self._track_states = self.tracked_assignment = None
        self.tracked_present = self.tracked_rows = None
        self._init_identity_bank(identity_capacity)

    @property
    def theta(self):
        """smooth_pose's state without identities, under the reference's name (notebooks/infer.py:571-581): None before the
        stream's first frame, else its EMA [4,4] (a view of the state row, which the next scan updates).  Reading it reads a
        device flag, so it may synchronise: nothing on the batched paths does.  Assigning None restarts the stream."""
        return self._stream.theta[0] if int(self._stream.theta_has[0]) else None

    @theta.setter
    def theta(self, value):
        if value is None:
            self._stream.restart(pose_ema=True)
        else:
            self._stream.theta[0].copy_(value.reshape(4, 4))
            self._stream.theta_has.fill_(1)

    def _capture(self, seq):
        """with use_graphs: replay the _sequence method `seq` from a hipGraph from its (1 + _graph_eager_calls)-th call of an
        input signature on"""
        if self.use_graphs:
            self._graphed[seq.key] = graphs.Graphed(functools.partial(seq.eager, self), eager_calls=self._graph_eager_calls)

    # ------------------------------------------------------------------------------------------------------
    def _native_embedders(self, found, head_pose_regressor_path):
        """IdtEmbed / ExpressionEmbed from the checkpoint (va.py:161,165), HeadPoseRegressor from its own file (va.py:258)"""
        out = {}
        sd = self.model_dict
        has = lambda p: any(k.startswith(p) for k in sd)
        if has("idt_embedder_nw.") or has("expression_embedder_nw."):
            ecfg = emb_mod.embedder_config(found, released='norm_layer_type' not in found)
            self.embedder_cfg = ecfg
            if has("idt_embedder_nw."):
                out['idt_embedder'] = emb_mod.IdtEmbed(sd, ecfg, self.device)
            if has("expression_embedder_nw."):
                out['expression_embedder'] = emb_mod.ExpressionEmbed(sd, ecfg, self.device)
        path = head_pose_regressor_path or found.get('head_pose_regressor_path')
        if head_pose_regressor_path is not None or (path and os.path.isfile(str(path))):
            out['head_pose_regressor'] = emb_mod.HeadPoseRegressor(torch.load(path, map_location='cpu'), self.device)
        return out

    def _set_source_cache(self, canonical=None, idt_embed=None, canonical_cl=None):
        """per-identity cache; with graphs the captured sequences hold the buffer addresses, so a new identity is copied
        INTO the existing buffers instead of rebinding them.  canonical: the NCDHW volume (kept as target_latent_volume and
        repacked); canonical_cl: a volume that is channels-last already -- a view of a bank row, cloned where it is bound"""
        if idt_embed is not None:
            if self.use_graphs and self.idt_embed is not None and self.idt_embed.shape == idt_embed.shape:
                self.idt_embed.copy_(idt_embed)
            else:
                self.idt_embed = idt_embed.clone() if self.use_graphs else idt_embed
        if canonical is not None:
            self.target_latent_volume = canonical
        cl = canonical_cl if canonical is None else self.hot_path.prepare_canonical(canonical)
        if cl is not None:
            if self.use_graphs and self._canonical_cl is not None and self._canonical_cl.shape == cl.shape:
                self._canonical_cl.copy_(cl)
            else:
                self._canonical_cl = cl if canonical is not None else cl.clone()

    # ---- identity bank --------------------------------------------------------------------------------------------
    def _init_identity_bank(self, capacity):
        """K slots preallocated on the device (captured graphs hold their addresses): channels-last canonical volumes
        [K,d,s,s,c] (25.2 MB per slot at the released config), idt_embed [K,C,es,es], source theta [K,4,4]"""
        if capacity < 0:
            raise ValueError("identity_capacity must be >= 0")
        self.identity_capacity = capacity
        self._bank_used = [False] * capacity
        # the controls' per-slot sources: the source expression [K,E] (_expr_bank allocates it, from the width of the first row
        # written) and the source (scale, rotation, translation) [K,9], and which slots have one
        self._bank_expr = self._bank_srt = None
        self._bank_expr_has, self._bank_srt_has = [False] * capacity, [False] * capacity
        if capacity == 0:
            self._bank_cl = self._bank_idt = self._bank_theta = self._bank_streams = None
            return
        c, d, s = self.cfg["latent_volume_channels"], self.cfg["latent_volume_depth"], self.cfg["latent_volume_size"]
        es = self.cfg["gen_embed_size"]
        f32 = dict(device=self.device, dtype=torch.float32)
        self._bank_cl = torch.zeros((capacity, d, s, s, c), **f32)
        self._bank_idt = torch.zeros((capacity, self.cfg["gen_max_channels"], es, es), **f32)
        self._bank_theta = torch.zeros((capacity, 4, 4), **f32)
        self._bank_srt = torch.zeros((capacity, 9), **f32)
        # each slot's own frame stream: smooth_pose's EMA, the controls' anchors and EMA
        self._bank_streams = control_streams.StreamStates(capacity, self.device)

    def _slot(self, slot, occupied=True):
        if self.identity_capacity == 0:
            raise ValueError("this wrapper has no identity bank: construct it with identity_capacity=K")
        slot = hostglue.bank_slot(slot, self.identity_capacity)
        if occupied and not self._bank_used[slot]:
            raise ValueError(f"slot {slot} holds no identity")
        return slot

    def _expr_bank(self, E):
        """the bank's expression rows, the slots' source expressions and their streams' anchor and EMA, allocated at the first use
        from the width E of the row at hand (a bank's `cfg` need not name it); every later row has that width"""
        self._bank_streams.expression(E)
        if self._bank_expr is None:
            self._bank_expr = torch.zeros((self.identity_capacity, E), device=self.device, dtype=torch.float32)

    def _bank_write(self, slot, canonical_cl, idt_embed, theta_src, expr_src=None, srt_src=None):
        if expr_src is not None:
            self._expr_bank(expr_src.numel())
        if idt_embed.numel() != self._bank_idt[slot].numel():
            raise ValueError(f"idt_embed {tuple(idt_embed.shape)} does not fit a slot {tuple(self._bank_idt.shape[1:])}")
        self._bank_cl[slot].copy_(canonical_cl.reshape(self._bank_cl.shape[1:]))
        self._bank_idt[slot].copy_(idt_embed.reshape(self._bank_idt.shape[1:]))
        self._bank_theta[slot].copy_(theta_src.reshape(4, 4))
        self._bank_used[slot] = True
        self._bank_srt_has[slot] = srt_src is not None       # (a slot whose source theta came as a matrix has no source pose)
        if srt_src is not None:
            self._bank_srt[slot].copy_(srt_src.reshape(9))
        self._bank_expr_has[slot] = expr_src is not None     # (a slot written without a source expression has no neutral)
        if expr_src is not None:
            self._bank_expr[slot].copy_(expr_src.reshape(-1))
        self._bank_streams.restart([slot], pose_ema=True, pose_anchor=True, expression=True)      # a new identity: new streams

    def store_identity(self, slot=None):
        """Copy the current identity (what forward(source_image=...) or share_source() left behind) into `slot` (None: the
        first free one); returns the slot"""
        if self.identity_capacity == 0:
            self._slot(0)                  # (raises: no bank)
        if self._canonical_cl is None or self.idt_embed is None:
            raise RuntimeError("no current identity: call forward with a source_image (or share_source) first")
        if self.pred_source_theta is None:
            raise RuntimeError("the current identity has no source theta")
        if slot is None:
            free = [k for k, used in enumerate(self._bank_used) if not used]
            if not free:
                raise ValueError(f"all {self.identity_capacity} identity slots are occupied: drop_identity one first")
            slot = free[0]
        slot = self._slot(slot, occupied=False)
        self._bank_write(slot, self._canonical_cl, self.idt_embed, self.pred_source_theta, self.pred_source_pose_embed,
                         self.pred_source_srt)
        return slot

    def load_identity(self, slot):
        """Make a stored identity current: forward(driver_image=...) then renders it.  Copied into the existing buffers as
        _set_source_cache does; target_latent_volume (NCDHW) is one repack of the channels-last slot."""
        slot = self._slot(slot)
        cl = self._bank_cl[slot:slot + 1]
        self.target_latent_volume = ops.volume_to_channels_first(cl)
        self._set_source_cache(canonical_cl=cl, idt_embed=self._bank_idt[slot:slot + 1].clone())
        self.pred_source_theta = self._bank_theta[slot:slot + 1].clone()
        self.pred_source_pose_embed = self._bank_expr[slot:slot + 1].clone() if self._bank_expr_has[slot] else None
        self.pred_source_srt = self._bank_srt[slot:slot + 1].clone() if self._bank_srt_has[slot] else None
        self._stream.restart(pose_anchor=True)    # (a new current identity: the single stream's relative pose starts again)

    def drop_identity(self, slot):
        slot = self._slot(slot)
        self._bank_used[slot] = self._bank_srt_has[slot] = self._bank_expr_has[slot] = False
        self._bank_streams.restart([slot], pose_ema=True, pose_anchor=True, expression=True)

    def reset_expression_state(self, slots=None):
        """Restart the expression controls' streams (the relative-transfer anchor and the expression EMA): slots=None clears the
        single-identity state and every slot's; otherwise only the given bank slots'"""
        self._restart(slots, expression=True)

    def reset_pose_state(self, slots=None):
        """Restart smooth_pose and the head-pose controls' relative transfer: slots=None clears the single-identity state
        (`self.theta`, the relative-pose anchor) and every slot's stream; otherwise only the streams of the given bank slots"""
        self._restart(slots, pose_ema=True, pose_anchor=True)

    def reset_crop_state(self, tracks=None):
        """Restart the crop tracker of animate_frames(boxes=) -- the EMA of tracking=dict(smooth=True) and the window that
        missing='hold' holds: tracks=None every track, otherwise the given ones (track p of boxes [N,P,4]; 0 for [N,4]).  The
        tracks are faces of the video, not identities: store_identity, drop_identity and the other bank events leave them alone.
        The tracks of animate_frames(detections=) are freed as well: their slots take the next new faces.  tracked_rows (tracking
        skip_absent=True) is forgotten."""
        self.tracked_rows = None
        if self._crop_streams is not None:
            self._crop_streams.restart(tracks)
        if getattr(self, "_track_states", None) is not None:
            self._track_states.restart(tracks)

    def _restart(self, slots, **which):
        """slots=None: the single stream and every slot's; a slot or several: theirs (StreamStates.restart)"""
        if slots is None:
            self._stream.restart(**which)
            if self._bank_streams is not None:
                self._bank_streams.restart(**which)
            return
        if not isinstance(slots, (list, tuple, range, torch.Tensor)):
            slots = [slots]
        rows = [self._slot(int(k), occupied=False) for k in slots]
        if rows:
            self._bank_streams.restart(rows, **which)

    def identities(self):
        """occupied slots, ascending"""
        return [k for k, used in enumerate(self._bank_used) if used]

    def share_identity(self, slot, src_rank=0):
        """Broadcast slot `slot` of rank `src_rank` into the same slot on every rank (one flat buffer,
        parallel.broadcast_source_cache)"""
        src = self.rank == src_rank
        slot = self._slot(slot, occupied=src)
        rows = {} if not src else dict(canonical_cl=self._bank_cl[slot:slot + 1], idt_embed=self._bank_idt[slot:slot + 1],
                                       theta_src=self._bank_theta[slot:slot + 1])
        if src and self._bank_expr_has[slot]:
            rows['expr_src'] = self._bank_expr[slot:slot + 1]
        if src:                                   # (a slot without a source pose sends a NaN row: the receivers read it once)
            rows['srt_src'] = self._bank_srt[slot:slot + 1] if self._bank_srt_has[slot] else torch.full((1, 9), float('nan'))
        cache = self._broadcast_rows(rows, 1, src_rank, 'canonical_cl', self._bank_cl.shape[1:])
        if not src:
            srt = cache["srt_src"]
            self._bank_write(slot, cache["canonical_cl"], cache["idt_embed"], cache["theta_src"], cache.get("expr_src"),
                             None if bool(torch.isnan(srt).any()) else srt)

    def _broadcast_rows(self, rows, n, src, volume, volume_shape, srt=True):
        """{volume, idt_embed, theta_src, expr_src, srt_src} of n identities from rank `src` (its `rows`; {} elsewhere) to every
        rank in one flat buffer, the shapes known on every rank: one collective, no host synchronisation
        (parallel.broadcast_source_cache).  expr_src, the source expressions, travels where the configuration names its width;
        srt_src, the source (scale, rotation, translation) rows [n,9], unless `srt` is False."""
        shapes = {volume: (n,) + tuple(volume_shape), 'idt_embed': (n,) + tuple(self._bank_idt.shape[1:]), 'theta_src': (n, 4, 4)}
        E = self.cfg.get("lpe_output_channels_expression")
        if E:
            shapes['expr_src'] = (n, int(E))
        if srt:
            shapes['srt_src'] = (n, 9)
        return parallel.broadcast_source_cache(rows, shapes=shapes, names=list(shapes), src=src, device=self.device,
                                               world=self.world, rank=self.rank, exchange_shapes=False)

    def enrol_identities(self, sources, source_masks=None, slots=None, crop=False, windows=None, batch_size=8,
                         custome_idt_embed=None, custome_source_pose_embed=None, custome_source_theta_embed=None,
                         frame_format="rgb8", colorspace="bt709", full_range=False):
        """Enrol K source identities into bank slots in chunks of `batch_size`: per chunk the mask products (ops.mul_mask), the
        embedders and HotPath.source_pass run at batch b, the canonical volumes go into their bank rows in one launch
        (ops.volume_to_channels_last_indexed) and the idt_embed / theta rows by device index copies -- no host synchronisation
        inside a chunk.  Identity k gets the semantics of forward(source_image=sources[k], source_mask=source_masks[k],
        crop=crop, custome_*=...[k]) followed by store_identity(slots[k]).
        sources: a list of images or a float tensor [K,3,H,W] (what forward takes, stacked), or uint8 frames [K,H,W,3] (host
        or device, animate_frames' input) with optional windows[k] = (x_lo, y_lo, side), cropped as animate_frames crops;
        with frame_format='nv12' the uint8 frames are NV12 [K, 3H/2, W] (colorspace, full_range as in animate_frames).
        custome_*: K-row tensors; the theta as [K,4,4] or (scale, rotation, translation) of [K,3] each.
        slots=None takes the K lowest free slots; explicit slots may overwrite occupied ones.  Every check runs on the host
        before the first launch (ValueError; the bank is untouched).  The current identity is left as it is.
        On several ranks every rank calls with the same arguments: chunk j is sources [j * batch_size, (j + 1) * batch_size),
        rank r computes the chunks parallel.shard_range(n_chunks, r, world), and each chunk's owner broadcasts {canonical,
        idt_embed, theta} in one flat buffer, from which every rank, the owner included, writes its rows -- the bank is the
        same bit for bit on every rank and for any number of ranks.  Returns the slots in the order of `sources`."""
        with torch.no_grad():
            plan = self._enrolment_checks(sources, source_masks, slots, crop, windows, batch_size, custome_idt_embed,
                                          custome_source_pose_embed, custome_source_theta_embed, frame_format, colorspace,
                                          full_range)
            return self._enrol_identities(plan, sources, crop, custome_idt_embed, custome_source_pose_embed,
                                          custome_source_theta_embed)

    def _enrolment_checks(self, sources, source_masks, slots, crop, windows, batch_size, custome_idt_embed,
                          custome_source_pose_embed, custome_source_theta_embed, frame_format="rgb8", colorspace="bt709",
                          full_range=False):
        """enrol_identities on the host, before anything is launched -> what the device part needs beside the arguments"""
        S = self.cfg["image_size"]
        frames_mod.check_format(frame_format, colorspace)
        video = isinstance(sources, torch.Tensor) and sources.dtype in (torch.uint8, ops.yuv420_dtype(frame_format))
        if frame_format != "rgb8":
            if not video:
                raise ValueError(f"frame_format={frame_format!r} describes {str(ops.yuv420_dtype(frame_format)).replace('torch.', '')} "
                                 f"frames [K, 3H/2, W]")
            frames_mod.check_frames(sources, frame_format)
        if isinstance(sources, torch.Tensor):
            if video and frame_format == "rgb8" and (sources.dim() != 4 or sources.shape[-1] != 3):
                raise ValueError(f"uint8 sources must be frames [K,H,W,3], got {tuple(sources.shape)}")
            if not video and (sources.dim() != 4 or sources.shape[1] < 3):
                raise ValueError(f"float sources must be [K,3,H,W], got {tuple(sources.shape)}")
            K = sources.shape[0]
        elif isinstance(sources, (list, tuple)):
            K = len(sources)
        else:
            raise ValueError("sources: a list of images, a float tensor [K,3,H,W] or uint8 frames [K,H,W,3]")
        slots, chunks, owners = hostglue.enrolment_plan(self._bank_used, K, slots, batch_size, self.world)
        if video and crop:
            raise ValueError("uint8 frames are cropped by windows= (crop=True detects faces in images)")
        if windows is not None and not video:
            raise ValueError("windows= crops uint8 frames [K,H,W,3]")
        win_host = None
        if windows is not None:
            H, W = frames_mod.frame_size(sources, frame_format)
            win_host = ops.windows_host(frames_mod.square_windows(windows), K, (W, H), "crop", "sources")
        parsing = 'face_parsing' in self.embedders
        ms = None
        if source_masks is not None:
            ms = [source_masks[i] for i in range(source_masks.shape[0])] if isinstance(source_masks, torch.Tensor) else list(source_masks)
            if len(ms) != K:
                raise ValueError(f"{len(ms)} source masks for {K} sources")
            if any(m.numel() != S * S for m in ms):
                raise ValueError(f"a source mask is not one {S}x{S} plane")
        elif not parsing:
            raise ValueError("enrolment needs source_masks= (or a 'face_parsing' embedder): the reference masks the source with "
                             "BiSeNet face parsing (infer.py:410-417)")

        def rows(t, what, row_shape=None):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] != K:
                raise ValueError(f"{what}: expected a tensor of {K} rows, got {getattr(t, 'shape', type(t))}")
            if row_shape is not None and tuple(t.shape[1:]) != tuple(row_shape):
                raise ValueError(f"{what}: rows {tuple(t.shape[1:])}, expected {tuple(row_shape)}")
            return t
        rows(custome_idt_embed, 'custome_idt_embed')
        if custome_idt_embed is not None and custome_idt_embed[0].numel() != self._bank_idt[0].numel():
            raise ValueError(f"custome_idt_embed rows {tuple(custome_idt_embed.shape[1:])} do not fit a slot "
                             f"{tuple(self._bank_idt.shape[1:])}")
        rows(custome_source_pose_embed, 'custome_source_pose_embed')
        theta_in = custome_source_theta_embed
        if theta_in is not None:
            if isinstance(theta_in, torch.Tensor):
                rows(theta_in, 'custome_source_theta_embed', (4, 4))
            elif isinstance(theta_in, (tuple, list)) and len(theta_in) == 3:
                for t in theta_in:
                    rows(t, 'custome_source_theta_embed (scale, rotation, translation)', (3,))
            else:
                raise ValueError("custome_source_theta_embed: a [K,4,4] tensor or (scale, rotation, translation)")
        if custome_idt_embed is None:
            self._need('idt_embedder', 'enrolment')
        if theta_in is None:
            self._need('head_pose_regressor', 'enrolment')
        if custome_source_pose_embed is None:
            self._need('expression_embedder', 'enrolment')
        images = None if video else (list(sources) if isinstance(sources, (list, tuple)) else [sources[i] for i in range(K)])
        boxes = None
        if crop and 'cropper' not in self.embedders:
            # forward(crop=True) renders a zero crop where no face was found: found here, before anything is launched
            det = self._need('face_detector', 'crop=True')
            boxes = []
            for i, img in enumerate(images):
                rel = det(img)
                t = self.convert_to_tensor(img)[0, :3]
                face = None if rel is None else hostglue.detection_to_face(*rel, t.shape[2], t.shape[1])
                win = hostglue.crop_window(face, t.shape[2], t.shape[1])
                if win is None:
                    raise ValueError(f"source {i}: no face found (forward would render a zero crop for it; nothing was enrolled)")
                boxes.append((t, win))
        return Namespace(slots=slots, chunks=chunks, owners=owners, video=video, win_host=win_host, masks=ms, images=images,
                         boxes=boxes, parsing=parsing, frame_format=(frame_format, colorspace, bool(full_range)))

    def _enrol_identities(self, plan, sources, crop, custome_idt_embed, custome_source_pose_embed, theta_in):
        """the device part: inputs uploaded once, then chunk by chunk without a host synchronisation"""
        S, dev = self.cfg["image_size"], self.device
        rows32 = torch.tensor(plan.slots, dtype=torch.int32).to(dev)
        rows64 = rows32.long()
        masks = None if plan.masks is None else torch.cat([m.reshape(1, 1, S, S) for m in plan.masks]).to(dev).float().contiguous()
        up = lambda t: None if t is None else t.to(dev).float().contiguous()
        idt_all, pose_all = up(custome_idt_embed), up(custome_source_pose_embed)
        theta_all, srt_all = (None, None) if theta_in is None else self._theta_from(theta_in)
        srt_all = None if srt_all is None else self._srt9(srt_all)
        has_srt = not isinstance(theta_in, torch.Tensor)        # (a 4x4 source theta: the identity has no source pose)
        if plan.video:
            u8 = sources.to(dev).contiguous()
            win_dev = None if plan.win_host is None else plan.win_host.to(dev)
        elif not crop:
            crops_all = torch.cat([self._prepare_image(img) for img in plan.images])          # (as forward, per image)
        elif plan.boxes is None:
            crops_all = self.embedders['cropper'](plan.images).to(dev)
        else:
            crops_all = torch.cat([ops.resize2d(t[None].to(dev).float().contiguous(), (S, S), "bicubic",
                                                window=(x_lo, y_lo, side, side), clamp01=True) for t, (x_lo, y_lo, side, _) in plan.boxes])
        es_shape = tuple(self._bank_idt.shape[1:])

        def compute(a, b):
            if plan.video:
                crop_img = frames_mod.crops_of(u8[a:b], S, None if win_dev is None else win_dev[a:b], *plan.frame_format)   # one launch per chunk
            else:
                crop_img = crops_all[a:b].float().contiguous()
            m = None if masks is None else masks[a:b]
            face = (self.embedders['face_parsing'](crop_img) > 0.6).float().contiguous() if plan.parsing else m   # infer.py:408-411
            crop_m = ops.mul_mask(crop_img, face)
            masked = ops.mul_mask(crop_m, m if m is not None else face)
            idt = idt_all[a:b] if idt_all is not None else self._need('idt_embedder', 'enrolment')(masked)
            if theta_all is not None:
                theta, srt = theta_all[a:b], None if srt_all is None else srt_all[a:b]
            else:
                theta, *srt = self._head_pose(crop_m)
                # (a regressor that returns no (scale, rotation, translation): NaN rows, which the controls would hand on)
                srt = self._srt9(srt) if len(srt) == 3 and all(t is not None for t in srt) else torch.full((b - a, 9), float('nan'),
                                                                                                          device=dev)
            pose = pose_all[a:b] if pose_all is not None else self._expression(crop_m, theta, 'enrolment')[0]
            theta = theta.float().contiguous()
            canonical = self.hot_path.source_pass(masked, idt.float().contiguous(), pose.float().contiguous(), theta)
            part = dict(canonical=canonical, idt_embed=idt.float().reshape((b - a,) + es_shape), theta_src=theta.reshape(b - a, 4, 4),
                        expr_src=pose.float().reshape(b - a, -1))
            if has_srt:
                part["srt_src"] = srt
            return part

        def write(part, a, b):
            ops.volume_to_channels_last_indexed(part["canonical"], self._bank_cl, rows32[a:b])
            self._bank_idt.index_copy_(0, rows64[a:b], part["idt_embed"])
            self._bank_theta.index_copy_(0, rows64[a:b], part["theta_src"])
            if "expr_src" in part:
                self._expr_bank(part["expr_src"].shape[1])
                self._bank_expr.index_copy_(0, rows64[a:b], part["expr_src"])
            if has_srt:
                self._bank_srt.index_copy_(0, rows64[a:b], part["srt_src"])

        if self.world == 1:
            for a, b in plan.chunks:
                write(compute(a, b), a, b)
        else:
            # each rank computes its own chunks first, then every chunk travels from its owner, in chunk order
            mine = {j: compute(a, b) for j, (a, b) in enumerate(plan.chunks) if plan.owners[j] == self.rank}
            c, d, s = self.cfg["latent_volume_channels"], self.cfg["latent_volume_depth"], self.cfg["latent_volume_size"]
            for j, (a, b) in enumerate(plan.chunks):
                write(self._broadcast_rows(mine.pop(j, {}), b - a, plan.owners[j], 'canonical', (c, d, s, s), srt=has_srt), a, b)
        for k in plan.slots:
            self._bank_used[k] = True
            self._bank_expr_has[k] = self._bank_expr is not None
            self._bank_srt_has[k] = has_srt
        self._bank_streams.restart(rows64, pose_ema=True, pose_anchor=True, expression=True)      # new identities: new streams
        return plan.slots

    def _frame_identities(self, identities, n=None):
        """per-frame slots -> int32 host tensor, every slot checked on the host (the device never sees an unknown slot)"""
        if self.identity_capacity == 0:
            raise ValueError("identities= needs an identity bank: construct the wrapper with identity_capacity=K")
        ids = torch.as_tensor(identities).detach().cpu()
        if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise ValueError("identities must be a 1-D integer sequence of slots, one per frame")
        if n is not None and ids.shape[0] != n:
            raise ValueError(f"identities has {ids.shape[0]} entries for {n} frames")
        for k in sorted(set(ids.tolist())):
            self._slot(int(k))
        return ids.to(torch.int32)

    # ---- stage 2 in the video path -----------------------------------------------------------------------------------
    def attach_stage2(self, stage2):
        """Give animate() / animate_frames() the refinement model their refine=True runs after every rendered batch: a
        stage2.InferenceWrapper (its 'matting' / 'face_parsing' embedders and its `cloth` flag then supply the masks, as in its
        own forward()) or a bare stage2.Stage2 (masks from refine_masks=); None detaches.  With use_graphs the stage-2 pass
        (Stage2.refine_frames) is captured per batch shape under the policy of the stage-1 sequences: first call of a shape
        eager, second captured, later ones replayed.  The mask callables are third-party nets and always run eagerly, between
        the two graphs.  In the 'f16x2' mode a stage-2 pass clears the device's range-check words, so ops.overflow_events() of
        the stage-1 pass of the same batch is gone once the batch is yielded."""
        from . import stage2 as s2
        for k in ('stage2_u8', 'stage2_f32'):
            self._graphed.pop(k, None)
        self._stage2 = self._stage2_wrapper = None
        if stage2 is None:
            return
        model = stage2.model_two if isinstance(stage2, s2.InferenceWrapper) else stage2
        if not isinstance(model, s2.Stage2):
            raise TypeError("attach_stage2 takes a stage2.InferenceWrapper, a stage2.Stage2 or None")
        self._stage2 = model
        self._stage2_wrapper = stage2 if model is not stage2 else None
        self._capture(type(self)._refine_u8)
        self._capture(type(self)._refine_f32)

    def _refine_plan(self, refine, refine_masks):
        """the checks of refine=True, before anything is launched -> None (no refinement) or the callable img [b,3,S2,S2] ->
        (mask, face_mask) that serves the masks of a batch"""
        if not refine:
            if refine_masks is not None:
                raise ValueError("refine_masks= belongs to refine=True")
            return None
        model = self._stage2
        if model is None:
            raise ValueError("refine=True needs a stage-2 model: attach_stage2(stage2.InferenceWrapper(...)) first")
        if torch.device(model.device) != torch.device(self.device):
            raise ValueError(f"the attached stage-2 model is on {model.device}, this wrapper renders on {self.device}")
        if refine_masks is not None:
            if not callable(refine_masks):
                raise ValueError("refine_masks: a callable img [b,3,S2,S2] -> (mask [b,1,S2,S2], face_mask [b,1,S2,S2])")
            return refine_masks
        w2 = self._stage2_wrapper
        emb = {} if w2 is None else w2.embedders
        cloth = bool(w2 is not None and w2.cloth)
        for name in ('matting',) if cloth else ('matting', 'face_parsing'):
            if not callable(emb.get(name)):
                raise ValueError(f"refine=True needs the '{name}' callable of the attached stage-2 wrapper "
                                 f"(stage2.InferenceWrapper(embedders={{'{name}': fn}})) or refine_masks=")
        matting, parsing = emb['matting'], emb.get('face_parsing')

        def masks_of(img):                                                       # stage2.InferenceWrapper.forward's choice
            mask = matting(img)
            return mask, (torch.ones_like(mask) if cloth else parsing(img))      # infer_s2.py:366-368
        return masks_of

    def _refine(self, img, masks_of, out):
        """stage 1's image of a batch -> the refined batch: bilinear resize to output_size_s2 where the sizes differ
        (infer_s2.py:360-362), the mask callables (eager), the stage-2 pass (captured with use_graphs).  out 'u8' | 'f32'"""
        model = self._stage2
        S2 = model.cfg["output_size_s2"]
        if img.shape[-1] != S2 or img.shape[-2] != S2:
            img = ops.resize2d(img, (S2, S2), "bilinear")
        mask, face = masks_of(img)
        mask = mask.to(self.device).float().contiguous()
        face = face.to(self.device).float().contiguous()
        return (self._refine_u8 if out == "u8" else self._refine_f32)(img, mask, face)

    @_sequence('stage2_u8')
    def _refine_u8(self, img, mask, face):
        return self._stage2.refine_frames(img, mask, face, "u8")

    @_sequence('stage2_f32')
    def _refine_f32(self, img, mask, face):
        return self._stage2.refine_frames(img, mask, face, "f32")

    @_sequence('driver')
    def _drive(self, pose, theta):
        return self.hot_path.driver_pass(self._canonical_cl, self.idt_embed, pose, theta)

    @_sequence('driver_bank')
    def _drive_bank(self, pose, theta, ident):
        """reads the bank buffers (fixed addresses) and the per-frame slots (an input of the graph): new indices and newly
        stored identities take effect on replay"""
        return self.hot_path.driver_pass(self._bank_cl, self._bank_idt, pose, theta, identity=ident)

    @_sequence('head_pose_regressor')
    def _head_pose(self, crop):
        return self._need('head_pose_regressor', 'a driver call')(crop, True)

    @_sequence('expression_embedder')
    def _expression_pass(self, crop, theta):
        fn = self.embedders['expression_embedder']
        return fn(crop, theta, True)[:2] if isinstance(fn, emb_mod.ExpressionEmbed) else fn(crop, theta)

    def _expression(self, crop, theta, what):
        """-> (pose_embed, aligned crop or None).  The aligned 128^2 crop is what the reference exposes as
        `target_img_align` (expression_embedder.py:233, infer.py:608); a user-supplied callable may return either the
        embedding alone or a tuple (embedding, aligned, ...)."""
        self._need('expression_embedder', what)
        out = self._expression_pass(crop, theta.float().contiguous())
        if isinstance(out, (tuple, list)):
            return out[0], (out[1] if len(out) > 1 else None)
        return out, None

    def _need(self, name, what):
        fn = self.embedders.get(name)
        if fn is None:
            raise RuntimeError(
                f"{what} needs the '{name}' network: it was not passed via InferenceWrapper(embedders={{'{name}': callable}}) "
                f"and, for the embedders this package runs itself, its weights were not found (checkpoint keys / "
                f"head_pose_regressor_path); the custome_* arguments can supply its output instead")
        return fn

    def convert_to_tensor(self, image):
        """infer.py:211-223: PIL / ndarray / tensor -> float tensor [B,3,H,W] in [0,1]"""
        import numpy as np
        if isinstance(image, torch.Tensor):
            t = image.float()
            return t[None] if t.dim() == 3 else t
        if isinstance(image, (list, tuple)):
            return torch.cat([self.convert_to_tensor(i) for i in image])
        arr = np.asarray(image)
        t = torch.from_numpy(arr.copy())
        if t.dtype == torch.uint8:
            t = t.float() / 255.0
        t = t.float()
        if t.dim() == 2:
            t = t[..., None].expand(-1, -1, 3)
        return t.permute(2, 0, 1)[None]

    def _prepare_image(self, image):
        S = self.cfg["image_size"]
        t = self.convert_to_tensor(image)[:, :3].to(self.device).contiguous()
        if t.shape[-2:] != (S, S):
            t = ops.resize2d(t, (S, S), "bicubic")                                  # infer.py:399-401
        return t

    def crop_image(self, image, faces, use_smoothed_crop=False, scale=1):
        """notebooks/infer.py:301-352: square window around each face box (host arithmetic, emoportraits_amd/hostglue.py),
        read in place from the frame and resized to image_size with the bicubic kernel, clipped to [0,1].
        image: list of [3,H,W] tensors or a [B,3,H,W] tensor; faces: list of (x0, y0, x1, y1) or None.
        Returns (crops [B,3,S,S] on the device, face_check, face_scale_stats) like the reference."""
        import numpy as np
        S = self.cfg["image_size"]
        if use_smoothed_crop and self._crop_tracker is None:
            self._crop_tracker = hostglue.CropTracker(self.momentum, self.fixed_bounding_box)
        crops, face_check, face_scale_stats = [], np.ones(len(image), dtype=bool), []
        for b, face in enumerate(faces):
            frame = image[b]
            win = hostglue.crop_window(face, frame.shape[2], frame.shape[1],
                                       self._crop_tracker if use_smoothed_crop else None, scale)
            if win is None:
                face_check[b] = False
                crops.append(torch.zeros((1, 3, S, S), device=self.device))
                face_scale_stats.append(0)
                continue
            x_lo, y_lo, side, face_scale = win
            frame = frame[None, :3].to(self.device).float().contiguous()
            crops.append(ops.resize2d(frame, (S, S), "bicubic", window=(x_lo, y_lo, side, side), clamp01=True))
            face_scale_stats.append(face_scale)
        if self._crop_tracker is not None:
            self.center, self.size = self._crop_tracker.center, self._crop_tracker.size
        return torch.cat(crops), face_check, face_scale_stats

    def _detect_and_crop(self, images):
        """crop=True (notebooks/infer.py:376-393, :515-546): face detector (third party: mediapipe in the reference, here the
        'face_detector' callable: PIL image -> relative box (xmin, ymin, width, height) or None) + crop_image.  A 'cropper'
        callable, if given, replaces the whole step."""
        if 'cropper' in self.embedders:
            return self.embedders['cropper'](images).to(self.device)
        det = self._need('face_detector', 'crop=True')
        images = images if isinstance(images, (list, tuple)) else [images]
        faces, tensors = [], []
        for img in images:
            rel = det(img)
            t = self.convert_to_tensor(img)[0, :3]
            faces.append(None if rel is None else hostglue.detection_to_face(*rel, t.shape[2], t.shape[1]))
            tensors.append(t)
        crops, self.face_check, self.face_scale_stats = self.crop_image(tensors, faces)
        return crops

    def get_mixing_theta(self, source_theta, target_theta):
        """notebooks/infer.py:686-736 (host scipy polar decomposition there as well)"""
        mixed = hostglue.mixing_theta(source_theta.detach().cpu().numpy(), target_theta.detach().cpu().numpy(), self.mix_old)
        return torch.from_numpy(mixed).float().to(self.device)

    def _theta_from(self, embed):
        """(scale, rotation, translation) as the reference's custome_target_theta_embed (-> get_transform_matrix,
        infer.py:565-566), or an already formed [B,4,4] theta tensor (extension)"""
        if isinstance(embed, torch.Tensor):
            return embed.to(self.device).float().contiguous(), None
        srt = tuple(t.to(self.device).float().contiguous() for t in embed)
        return ops.pose_theta(*srt), srt

    def _srt9(self, srt):
        """(scale [n,1] or [n,3], rotation [n,3], translation [n,3]) -> one [n,9] row per sample, a one-column scale broadcast"""
        scale, rotation, translation = (t.to(self.device).float() for t in srt)
        return torch.cat([scale.expand(scale.shape[0], 3), rotation, translation], dim=1).contiguous()

    def _source_theta(self, what):
        theta = self.pred_source_theta
        if theta is None:
            raise RuntimeError(f"{what} needs the current identity's source theta: call forward with a source_image (or "
                               f"share_source) first")
        return theta.reshape(1, 4, 4).float().contiguous()

    def _pose_controls(self, theta, ids_dev, mix, mix_old, smooth, r0=0, masks=None):
        """forward()'s order (infer.py:568-581) on a batch of driver thetas IN FRAME ORDER, on the device: mix against each
        frame's identity (bank slot ids_dev[i], or the current identity), then smooth_pose (ops.theta_ema_scan, bit for bit
        hostglue.ema_scan = the reference's per-frame loop) -- with a bank one stream per slot, else the single stream, whose
        state (`self.theta` reads it) carries from call to call as the reference's does.  masks: where the streams follow face
        tracks, the chunk's row masks (control_streams.row_masks), and r0 the first row's index in the call"""
        theta = theta.to(self.device).float().contiguous()
        if theta.shape[0] == 0:
            return theta
        if mix:
            if ids_dev is None:
                theta = ops.mixing_theta(theta, self._source_theta('mix=True'), None, mix_old)
            else:
                theta = ops.mixing_theta(theta, self._bank_theta, ids_dev, mix_old)
        if smooth:
            st = self._stream if ids_dev is None else self._bank_streams
            masks = control_streams.row_masks(masks, r0, theta.shape[0])
            theta = ops.theta_ema_scan(theta, ids_dev, st.theta, st.theta_has, self.pose_momentum, **masks)
        return theta

    def _expression_controls(self, values, ids_dev, ex, r0, masks=None):
        """The expression controls `ex` (control_streams.expression_plan) on values [m,E] = the rows r0 ... of the call IN FRAME
        ORDER, one launch (ops.expression_controls, bit for bit hostglue.expression_controls): every row about its identity's source
        expression (bank slot ids_dev[i], or the current identity's), and for relative / smooth within its slot's stream -- without
        identities the one stream of the current identity (_stream), carried from call to call as smooth_pose's is"""
        values = values.to(self.device).float().contiguous()
        m = values.shape[0]
        if m == 0 or not (ex.step1 or ex.scan or ex.offset is not None):          # (an override alone: nothing to compute)
            return values
        gain = control_streams.rows_of(ex.gain, r0, m, 'expression gain')
        offset = control_streams.rows_of(ex.offset, r0, m, 'expression offset', whole=1)
        if not (ex.step1 or ex.scan):                                            # (an offset alone: no source, no stream)
            return ops.expression_controls(values, offset=offset)
        st = self._stream if ids_dev is None else self._bank_streams
        if ids_dev is None:
            st.expression(values.shape[1])
            neutral = self.pred_source_pose_embed.to(self.device).float().reshape(1, -1).contiguous() if ex.step1 else None
        else:
            self._expr_bank(values.shape[1])
            neutral = self._bank_expr if ex.step1 else None
        masks = control_streams.row_masks(masks, r0, m) if ex.scan else {}       # (masks: _pose_controls'; no stream state, none)
        return ops.expression_controls(values, ids_dev, neutral, gain, offset, st.expr_anchor, st.expr_anchor_has, st.expr_ema,
                                       st.expr_ema_has, ex.relative, ex.momentum, **masks)

    def _head_pose_controls(self, srt, ids_dev, hp, r0, masks=None):
        """The head-pose controls `hp` (control_streams.head_pose_plan) on srt = (scale, rotation, translation) of the rows r0 ... of
        the call IN FRAME ORDER, one launch (ops.head_pose_controls, bit for bit hostglue.head_pose_controls) -> (the edited rows
        [m,9], their theta [m,4,4]): every row about its identity's source pose (bank slot ids_dev[i], or the current identity's),
        and for `relative` within its slot's stream -- without identities the one stream of the current identity (_stream), whose
        anchor carries from call to call.  pred_target_srt is left as the edited triple."""
        if srt is None or len(srt) != 3 or any(t is None for t in srt):
            raise RuntimeError("head_pose= edits the (scale, rotation, translation) of the head-pose regressor, which returned none: "
                               "a 'head_pose_regressor' callable must return (theta, scale, rotation, translation)")
        scale, rotation, translation = (t.to(self.device).float().contiguous() for t in srt)
        m = scale.shape[0]
        if m == 0:
            return torch.empty((0, 9), device=self.device), torch.empty((0, 4, 4), device=self.device)

        gain, zoom = (control_streams.rows_of(getattr(hp, name), r0, m, f'head_pose {name}', whole=0) for name in ('gain', 'zoom'))
        rot, trans = (control_streams.rows_of(getattr(hp, name), r0, m, f'head_pose {name}', whole=1)
                      for name in ('rotation_offset', 'translation_offset'))
        st, source = self._stream if ids_dev is None else self._bank_streams, None
        if hp.step1:
            source = self._bank_srt if ids_dev is not None else self.pred_source_srt.to(self.device).float().reshape(1, 9).contiguous()
        # (without step1 there is no source and no stream: every row by itself; only `relative` has a state that follows the tracks)
        masks = control_streams.row_masks(masks, r0, m) if hp.relative else {}           # (masks: _pose_controls')
        out = ops.head_pose_controls(scale, rotation, translation, ids_dev if hp.step1 else None, source, gain, rot, trans, zoom,
                                     st.pose_anchor, st.pose_anchor_has, hp.relative, hp.frontal, **masks)
        self.pred_target_srt = tuple(out[0][:, i:i + 3] for i in (0, 3, 6))
        return out

    def _control_plans(self, expression, head_pose, n_rows, ids, where, target_theta, faces=False):
        """the checks of expression= and head_pose=, before anything is launched -> (ex, hp): what _expression_controls and
        _head_pose_controls need, None for a keyword that asks for nothing (control_streams.expression_plan, head_pose_plan)"""
        ex = control_streams.expression_plan(expression, n_rows, ids, where, faces, self.device, self.pred_source_pose_embed,
                                             self._bank_expr_has, None if self._bank_expr is None else self._bank_expr.shape[1])
        hp = control_streams.head_pose_plan(head_pose, n_rows, ids, where, target_theta, faces, self.device, self.pred_source_srt,
                                            self._bank_srt_has)
        return ex, hp

    def _render_theta(self, theta, ids_dev, target_theta):
        """target_theta=False: the frame is rendered in its identity's own head pose (infer.py:584), a device-side gather"""
        if target_theta:
            return theta.float().contiguous()
        if ids_dev is None:
            return self._source_theta('target_theta=False').expand(theta.shape[0], 4, 4).contiguous()
        return self._bank_theta.index_select(0, ids_dev).contiguous()

    def to_image(self, img_u8_hwc):
        from PIL import Image
        return Image.fromarray(img_u8_hwc)

    # ------------------------------------------------------------------------------------------------------
    def forward(self, source_image=None, driver_image=None, source_mask=None, source_mask_add=0, driver_mask=None,
                crop=True, reset_tracking=False, smooth_pose=False, hard_normalize=False, soft_normalize=False,
                delta_yaw=None, delta_pitch=None, cloth=False, thetas_pass='', theta_n=0, target_theta=True,
                mix=False, mix_old=True, c_source_latent_volume=None, c_target_latent_volume=None,
                custome_target_pose_embed=None, custome_target_theta_embed=None, no_grad_infer=True,
                modnet_mask=False, custome_source_pose_embed=None, custome_source_theta_embed=None,
                custome_idt_embed=None):
        self.no_grad_infer = no_grad_infer
        self.target_theta = target_theta
        with torch.no_grad():
            if reset_tracking:
                self.center = self.size = self.delta_yaw = self.delta_pitch = None
                self._crop_tracker = None
                self.reset_crop_state()                    # (the reference resets `center` / `size`: the device tracker's too)
                self.reset_pose_state()
                self.reset_expression_state()
            self.mix, self.mix_old = mix, mix_old
            if delta_yaw is not None:
                self.delta_yaw = delta_yaw
            if delta_pitch is not None:
                self.delta_pitch = delta_pitch
            c, d, s = self.cfg["latent_volume_channels"], self.cfg["latent_volume_depth"], self.cfg["latent_volume_size"]

            if source_image is not None:
                if crop:
                    source_img_crop = self._detect_and_crop(source_image)
                else:
                    source_img_crop = self._prepare_image(source_image)
                self.source_image = source_image
                self.source_image_crop = source_img_crop
                # infer.py:408-420: the face-parsing mask (> 0.6) ALWAYS multiplies the crop; source_mask only replaces
                # source_img_mask.  Deviation, only when no 'face_parsing' network is installed (BiSeNet is third party):
                # source_mask then stands in for the face mask as well.
                if 'face_parsing' in self.embedders:
                    face_mask_source = (self.embedders['face_parsing'](source_img_crop) > 0.6).float()  # infer.py:408-411
                elif source_mask is not None:
                    face_mask_source = source_mask.to(self.device).float()
                else:
                    raise RuntimeError("a source call needs source_mask= (or a 'face_parsing' embedder): the reference "
                                       "masks the source with BiSeNet face parsing (infer.py:410-417)")
                source_img_mask = source_mask.to(self.device).float() if source_mask is not None else face_mask_source
                if modnet_mask:
                    source_img_mask = self._need('matting', 'modnet_mask=True')(source_img_crop)
                if source_mask_add:
                    source_img_mask = source_img_mask.clamp(max=1, min=0)
                source_img_crop = (source_img_crop * face_mask_source).float()
                self.source_img_crop_m = source_img_crop
                self.source_img_mask = source_img_mask
                masked = (source_img_crop * source_img_mask).contiguous()
                if custome_idt_embed is not None:
                    self._set_source_cache(idt_embed=custome_idt_embed.to(self.device).float().contiguous())
                else:
                    self._set_source_cache(idt_embed=self._need('idt_embedder', 'a source call')(masked))  # infer.py:432
                if custome_source_theta_embed is not None:
                    pred_source_theta, srt = self._theta_from(custome_source_theta_embed)
                else:
                    # (return_srt=True: the same theta, and the triple the head-pose controls work about)
                    out = self._need('head_pose_regressor', 'a source call')(source_img_crop, True)                      # :437
                    pred_source_theta, srt = (out[0], tuple(out[1:4])) if isinstance(out, (tuple, list)) else (out, None)
                self.pred_source_theta = pred_source_theta
                self.pred_source_srt = self._srt9(srt) if srt is not None and len(srt) == 3 and all(t is not None for t in srt) else None
                self._stream.restart(pose_anchor=True)     # a new source: the single stream's relative pose starts again
                if custome_source_pose_embed is not None:
                    source_pose_embed = custome_source_pose_embed.to(self.device).float().contiguous()
                else:
                    source_pose_embed, self.source_img_align = self._expression(source_img_crop, pred_source_theta,
                                                                                'a source call')
                self.pred_source_pose_embed = source_pose_embed
                self.source_img = source_img_crop

                hp = self.hot_path
                source_latents = hp.local_encoder(masked)                                              # infer.py:433
                emb = hp.embed(source_pose_embed, self.idt_embed)                                      # infer.py:459
                delta_xy = hp.xy_generator(emb)                                                        # infer.py:462
                vol = source_latents.view(1, c, d, s, s)
                if self.cfg["source_volume_num_blocks"] > 0:
                    vol = hp.volume_source(vol)                                                        # infer.py:490-491
                self.source_latent_volume = vol if c_source_latent_volume is None else \
                    c_source_latent_volume.to(self.device).float().contiguous()
                inv = ops.mat4_inverse(pred_source_theta.float().contiguous())                         # infer.py:443, on the device
                self._source_theta_inv = inv
                self.source_rotation_warp = ops.affine_grid3d(inv, (d, s, s))                          # infer.py:441-444
                self.source_xy_warp_resize = delta_xy
                rot = ops.grid_sample3d(ops.volume_to_channels_last(self.source_latent_volume), theta=inv, padding_mode=hp.pad,
                                        in_layout="ndhwc", out_layout="ndhwc")                         # infer.py:499-500
                tv = ops.grid_sample3d(rot, delta=delta_xy, padding_mode=hp.pad, in_layout="ndhwc", out_layout="ncdhw")
                self.target_latent_volume_1 = tv if c_target_latent_volume is None else \
                    c_target_latent_volume.to(self.device).float().contiguous()
                self._set_source_cache(canonical=hp.volume_process(self.target_latent_volume_1))      # infer.py:507

            if driver_image is None and custome_target_pose_embed is None:
                return None                                                                            # infer.py:644-646
            if self.target_latent_volume is None:
                raise RuntimeError("call forward with a source_image first (no cached canonical volume)")

            driver_img_crop = None
            if driver_image is not None:
                driver_img_crop = self._detect_and_crop(driver_image) if crop else self._prepare_image(driver_image)
            if custome_target_theta_embed is not None:                                                 # infer.py:565-566
                pred_target_theta, self.pred_target_srt = self._theta_from(custome_target_theta_embed)
            elif driver_img_crop is None:
                raise RuntimeError("forward(driver_image=None, custome_target_pose_embed=...) also needs "
                                   "custome_target_theta_embed=: without a driver frame there is nothing to regress the head "
                                   "pose from (the reference dereferences the missing crop at infer.py:562)")
            else:
                pred_target_theta, *srt = self._head_pose(driver_img_crop)                             # infer.py:562
                self.pred_target_srt = tuple(srt)
            if mix:                                                                                    # infer.py:568-569
                pred_target_theta = self.get_mixing_theta(self.pred_source_theta, pred_target_theta)
            if smooth_pose:                                                                            # infer.py:571-581
                pred_target_theta = self._pose_controls(pred_target_theta, None, False, mix_old, True)
            self.pred_target_theta = pred_target_theta
            theta_used = pred_target_theta if target_theta else self.pred_source_theta
            # the reference runs the expression embedder on every driver frame (infer.py:596-601) and only then overrides
            # its output (:603-604); target_img_align (:608) comes from that run
            self.target_img_align = None
            if driver_img_crop is None and custome_target_pose_embed is None:
                raise RuntimeError("forward(driver_image=None, custome_target_theta_embed=...) also needs "
                                   "custome_target_pose_embed=: without a driver frame there is no expression to embed")
            if driver_img_crop is not None and (custome_target_pose_embed is None or 'expression_embedder' in self.embedders):
                target_pose_embed, self.target_img_align = self._expression(driver_img_crop, pred_target_theta,
                                                                            'a driver call')
            if custome_target_pose_embed is not None:                                                  # infer.py:603-604
                target_pose_embed = custome_target_pose_embed.to(self.device).float().contiguous()
            self.target_pose_embed = target_pose_embed
            B = target_pose_embed.shape[0]
            if theta_used.shape[0] != B:
                theta_used = theta_used.expand(B, -1, -1)
            img = self._drive(target_pose_embed, theta_used.float().contiguous())                      # infer.py:612-637
            u8 = ops.pack_rgb8(img).cpu().numpy()                                                      # infer.py:641-643
            return [self.to_image(u8[i]) for i in range(B)], img

    __call__ = forward

    # ------------------------------------------------------------------------------------------------------
    def animate(self, target_pose_embeds, target_srt, batch_size=16, as_uint8=True, identities=None, mix=False, mix_old=True,
                target_theta=True, smooth_pose=False, smooth_per_identity=False, refine=False, refine_masks=None,
                out_format="rgb8", colorspace="bt709", full_range=False, expression=None, head_pose=None):
        """1 source -> N driver frames (the BASELINE metric).  Frames are sharded contiguously across ranks
        (SURVEY.md section 8e); each rank walks its shard in batches of `batch_size`.  Yields (first_frame_index, frames)
        with frames a uint8 [B,H,W,3] (or fp32 [B,3,H,W]) DEVICE tensor -- no host sync inside the loop.
        identities: slot of the identity bank per frame ([N], over the whole frame stream; each rank takes its slice) -- the
        frames of a batch may then belong to different identities.
        mix / mix_old / target_theta / smooth_pose: forward()'s pose controls (infer.py:568-584), all on the device.  mix keeps
        each frame's identity's face stretch (its bank slot's source theta, or the current identity's); target_theta=False
        renders in that identity's own head pose.  smooth_pose is a scan over the FRAME ORDER: every rank forms the thetas of
        the whole stream from target_srt (16 floats per frame) and scans them, then renders its own slice -- 1 rank and N ranks
        give the same frames.  Without identities the state is `self.theta` (carried from call to call, as in forward); with
        them, smooth_pose needs smooth_per_identity=True, and each slot then has its own stream.
        refine=True: every rendered batch goes through the attached stage-2 model (attach_stage2; see animate_frames) and the
        frames come out at its output_size_s2.
        out_format='nv12' (with as_uint8): the frames come out as NV12 uint8 [B, 3S/2, S] -- the fp32 image, refined or not,
        through ops.pack_yuv420 with `colorspace` ('bt709' | 'bt601') and `full_range` (see animate_frames).
        expression: an ExpressionControls (or a mapping with its fields) applied to target_pose_embeds on the device, see
        animate_frames; like smooth_pose, every rank runs it over the WHOLE stream in one launch and renders its slice, so the
        frames do not depend on batch_size or on the number of ranks.  override= is a ValueError: the expressions are inputs.
        head_pose: a HeadPoseControls (or a mapping with its fields) applied to target_srt on the device before theta is formed,
        see animate_frames; every rank edits the rows of the WHOLE stream in one launch (ops.head_pose_controls), mix and
        smooth_pose then work on the edited thetas, and each rank renders its slice."""
        N = target_pose_embeds.shape[0]
        frames_mod.check_format(out_format, colorspace, "out_format")
        if out_format != "rgb8" and not as_uint8:
            raise ValueError("as_uint8=False yields the fp32 image: it has no out_format")
        masks_of, ids = self._preflight(N, identities, mix, target_theta, smooth_pose, smooth_per_identity, refine, refine_masks)
        if out_format != "rgb8":
            self._yuv420_size(masks_of, out_format)
        ex, hp = self._control_plans(expression, head_pose, N, ids, 'animate', target_theta)
        out_kind = "f32" if not as_uint8 else ("u8" if out_format == "rgb8" else out_format)
        lo, hi = parallel.shard_range(N, self.rank, self.world)
        ids_dev = None if ids is None else ids[lo:hi].to(self.device)
        smoothed = edited = None
        if hp is not None and N > 0:
            edited = self._head_pose_controls(target_srt, None if ids is None else ids.to(self.device), hp, 0)[1]
        if smooth_pose and N > 0:
            theta = edited if edited is not None else ops.pose_theta(*[t.to(self.device).float().contiguous() for t in target_srt])
            smoothed = self._pose_controls(theta, None if ids is None else ids.to(self.device), mix, mix_old, True)[lo:hi]
        poses = None
        if ex is not None and N > 0:
            poses = self._expression_controls(target_pose_embeds, None if ids is None else ids.to(self.device), ex, 0)[lo:hi]
        for b0 in range(lo, hi, batch_size):
            b1 = min(b0 + batch_size, hi)
            pose = target_pose_embeds[b0:b1].to(self.device).float().contiguous() if poses is None else poses[b0 - lo:b1 - lo]
            ident = None if ids is None else ids_dev[b0 - lo:b1 - lo]
            if smoothed is not None:
                theta = smoothed[b0 - lo:b1 - lo]
            elif edited is not None:
                theta = self._pose_controls(edited[b0:b1], ident, mix, mix_old, False)
            else:
                srt = [t[b0:b1].to(self.device).float().contiguous() for t in target_srt]
                theta = self._pose_controls(ops.pose_theta(*srt), ident, mix, mix_old, False)
            yield b0, self._render(pose, theta, ident, target_theta, masks_of, out_kind, (colorspace, full_range))

    def _preflight(self, n_frames, identities, mix, target_theta, smooth_pose, smooth_per_identity, refine, refine_masks):
        """The checks of the keywords animate() and animate_frames() share, before anything is launched -> (masks_of, ids):
        _refine_plan's callable or None, and the per-frame slots as a host tensor or None (the current identity)"""
        masks_of = self._refine_plan(refine, refine_masks)
        # smooth_pose over a bank is one EMA stream PER SLOT, which is not the one stream of the driver video the single-identity
        # path smooths (frames of one driver clip spread over several identities would each skip the others' frames): the caller
        # asks for it explicitly
        if identities is not None and smooth_pose and not smooth_per_identity:
            raise ValueError("smooth_pose=True smooths one pose stream: with identities= pass smooth_per_identity=True to smooth "
                             "each identity's frames as a stream of its own")
        if identities is not None:
            return masks_of, self._frame_identities(identities, n_frames)
        if self._canonical_cl is None:
            raise RuntimeError("call forward with a source_image first")
        if mix or not target_theta:
            self._source_theta('mix=True' if mix else 'target_theta=False')
        return masks_of, None

    def _yuv420_size(self, masks_of, out_format):
        """YUV 4:2:0 frames have an even side: the size of the image that would be packed, checked before anything is launched"""
        name, S_out = ("image_size", self.cfg["image_size"]) if masks_of is None else ("output_size_s2", self._stage2.cfg["output_size_s2"])
        if S_out % 2:
            raise ValueError(f"{ops.yuv420_name(out_format)} output needs an even {name}, got {S_out}")

    def _render(self, pose, theta, ident, target_theta, masks_of, out, yuv=("bt709", False)):
        """The tail of a batch: the theta each frame is rendered with, the driver pass of the current identity or of the bank
        slots `ident`, stage 2 where masks_of is given -> uint8 [b,S,S,3] (out 'u8'), the fp32 image [b,3,S,S] ('f32') or
        that image in a YUV 4:2:0 layout ('nv12', 'yuv420p', 'p010', 'yuv420p10': ops.pack_yuv420 with yuv = (colorspace,
        full_range), [b,3S/2,S] of the format's dtype)"""
        theta = self._render_theta(theta, ident, target_theta)
        img = self._drive(pose, theta) if ident is None else self._drive_bank(pose, theta, ident)
        if out in frames_mod.YUV420:
            img = img if masks_of is None else self._refine(img, masks_of, "f32")
            return ops.pack_yuv420(img, out, *yuv)
        if masks_of is not None:
            return self._refine(img, masks_of, out)
        return ops.pack_rgb8(img) if out == "u8" else img

    # ------------------------------------------------------------------------------------------------------
    def _paste_matte(self, paste_matte, what):
        """paste_matte -> None | callable img [b,3,S,S] -> [b,1,S,S]  (True: embedders['matting']; a tensor: itself, for the one
        batch it belongs to)"""
        if paste_matte is None or paste_matte is False:
            return None
        if paste_matte is True:
            return self._need('matting', what)
        if isinstance(paste_matte, torch.Tensor):
            return lambda img: paste_matte
        if not callable(paste_matte):
            raise ValueError("paste_matte: None, True (embedders['matting']) or a callable img [b,3,S,S] -> [b,1,S,S]")
        return paste_matte

    def paste_back(self, frames_u8, rendered, windows=None, feather=0.0625, matte=None, frame_format="rgb8", colorspace="bt709",
                   full_range=False, faces=None):
        """The inverse of the crop: `rendered` [N,3,S,S] fp32 (the hot path's image, before emo_pack_rgb8) goes back into the
        frames the crops came from, frame i where its window windows[i] = (x_lo, y_lo, side) was -- resized to side x side
        (bicubic; antialiased when that shrinks it, down to S / 4), blended over the frame with a feathered edge of
        feather * side pixels and, if given, a matte ([N,1,S,S] in [0,1], a callable img -> matte, or True =
        embedders['matting']).  One launch (ops.paste_windows / emo_paste_windows_rgb8).
        frames_u8: uint8 [N,Hf,Wf,3], host or device; it is NOT modified (a host tensor is uploaded, a device tensor cloned).
        Returns the device uint8 [N,Hf,Wf,3].  feather = 1/16 of the window is a taste default, not a measured optimum.
        frame_format='nv12': frames_u8 is NV12 uint8 [N, 3Hf/2, Wf] and so is the result (ops.paste_windows_yuv420 /
        emo_paste_yuv420, with `colorspace` and `full_range` as in animate_frames).
        faces= instead of windows=: several faces per frame -- faces[i] = the (x_lo, y_lo, side) of frame i in paste order ([]: no
        face), `rendered` and the matte hold one row per face in that order, and the faces of a frame are pasted one over the
        other, the later one on top, still in one launch (emo_paste_faces_rgb8 / emo_paste_yuv420)."""
        frames_mod.check_format(frame_format, colorspace)
        if not isinstance(frames_u8, torch.Tensor):
            raise ValueError("frames must be a uint8 tensor")
        frames_mod.check_frames(frames_u8, frame_format)
        if (windows is None) == (faces is None):
            raise ValueError("paste_back takes either windows= (one per frame) or faces= (a list per frame)")
        fn = self._paste_matte(matte, 'matte=True')
        frame_of = None
        if faces is not None:
            wins, counts = frames_mod.flatten_faces(faces)
            if len(counts) != frames_u8.shape[0]:
                raise ValueError(f"faces has {len(counts)} entries for {frames_u8.shape[0]} frames")
            frame_of = [i for i, c in enumerate(counts) for _ in range(c)]
        else:
            wins = windows if isinstance(windows, torch.Tensor) and windows.is_cuda else frames_mod.square_windows(windows)
        img = rendered.to(self.device).float().contiguous()
        m = None if fn is None else fn(img).to(self.device).float().contiguous()
        full = frames_u8.to(self.device, copy=True)
        return frames_mod.paste_into(full if frame_format != "rgb8" else full.contiguous(), img, wins, feather, m, frame_format,
                                     colorspace, full_range, frame_of)

    def animate_frames(self, frames, batch_size=16, windows=None, ring=3, to_host=True, smooth_pose=False, identities=None,
                       mix=False, mix_old=True, target_theta=True, smooth_per_identity=False, paste_back=False, feather=0.0625,
                       paste_matte=None, as_uint8=True, refine=False, refine_masks=None, frame_format="rgb8", out_format=None,
                       colorspace="bt709", full_range=False, faces=None, expression=None, head_pose=None, boxes=None, tracking=None,
                       detections=None):
        """Video in -> video out, device resident (notebooks/infer.py:511-556, :562-601, :641-644 per
        frame there).  Per batch, all on the device and without a host synchronisation:
            byte -> fp32 CHW (emo_unpack_rgb8) -> crop windows read in place + bicubic resize to image_size, the whole batch in
            one launch (emo_resize2d_windows_f32) -> HeadPoseRegressor -> ExpressionEmbed -> hot path -> uint8 HWC.
        The driver-side matte (MODNet) of the reference is computed but unused with use_seg=False (infer.py:592-601): skipped.
        Frames are sharded contiguously across ranks as in animate().  Yields (first_frame_index, uint8 [b,S,S,3]).
        frames: uint8 [N,H,W,3] tensor (host, ideally pinned, or device) or an iterable of such chunks -- decoded video frames,
            uploaded as BYTES, span i + 1 beside the compute of span i (frames.uploaded).
        windows: windows[i] = (x_lo, y_lo, side) from the face detector + hostglue.crop_window, host arithmetic; None = whole
            frame.  (boxes= below takes the detector's boxes instead and forms the windows on the device.)
        to_host, ring: results go D2H into a ring of `ring` pinned buffers on a copy stream (frames.HostRing); a batch is
            yielded once ITS copy event has completed, i.e. the host only ever waits for a batch that is `ring - 1` batches
            behind the GPU.  What is yielded is a view of a pinned ring slot, valid ONLY until the generator is resumed (the
            next batch's copy may be queued into the same slot right away: consume or copy it before calling next()) -- or,
            with to_host=False, the device tensor.
        identities: slot of the identity bank per frame, over the whole frame stream (as in animate()).
        mix / mix_old / target_theta: forward()'s pose controls (infer.py:568-569, :584), per frame against that frame's
            identity, on the device (ops.mixing_theta; a gather of the bank's source thetas).  The order is forward()'s:
            regressed theta -> mix -> smooth_pose -> expression embedder -> render (with the source theta if
            target_theta=False).
        smooth_pose (infer.py:571-581) is a scan over the FRAME ORDER, so it runs before the frames are sharded (SURVEY.md
            section 8e): per chunk, every rank regresses the head pose of its own shard, the thetas (16 floats per frame) are
            gathered on every rank, the EMA runs once on the device over the whole chunk (ops.theta_ema_scan, bit for bit
            hostglue.ema_scan; state carried from chunk to chunk in `self.theta` exactly as the reference carries it from
            call to call), and only then does each rank render its shard with its slice of the smoothed thetas -- 1 rank and
            N ranks produce the same frames, and the pass needs no host synchronisation.  The crops of the shard stay
            resident between the two passes (3 MB per frame).
        smooth_per_identity: with identities, smooth_pose needs smooth_per_identity=True (else ValueError): each frame is then
            smoothed within its own identity's frame sequence, as if every identity had its own wrapper: one stream per slot,
            scanned over the whole gathered chunk on every rank, so the slot states stay identical across ranks;
            store_identity / drop_identity / reset_pose_state reset a slot's stream.
        paste_back=True: frames in -> FRAMES out.  Each batch's rendered fp32 image goes back into the batch's uploaded frame
            bytes where the crop windows were (paste_back(); one launch, emo_paste_windows_rgb8, in place of emo_pack_rgb8) and
            what is yielded is (first_frame_index, uint8 [b,Hf,Wf,3]); the pinned ring then holds full frames (a chunk of
            another frame size gets a new ring).  Needs `windows` (ValueError otherwise, before anything is launched), sides
            >= image_size / 4.  A host chunk's device copy is private and is pasted into in place; a device-resident chunk is
            cloned span by span: the caller's frames stay untouched.  With smooth_pose the head-pose pass keeps crops, not
            frames, so the render pass uploads the spans of a host chunk once more.  Each rank pastes its own shard: no
            collective.
        feather: width of the blended edge as a fraction of the window side (1/16: a taste default, not a measured optimum).
        paste_matte: None, a callable img [b,3,S,S] -> [b,1,S,S] in [0,1], or True = embedders['matting'].
        as_uint8=False (with to_host=False, without paste_back): the fp32 [b,3,S,S] device image itself, as animate() yields it
            -- what paste_back() takes as `rendered` (with captured graphs it is the graph's output buffer: consume or clone
            it before resuming the generator).
        refine=True, refine_masks: stage 2 in the path (attach_stage2 first; ValueError before anything is launched otherwise).
            Per batch, where the hot path returns its image: bilinear resize to the stage-2 model's output_size_s2 if that
            differs from image_size (infer_s2.py:360-362) -> the matte and the face mask of the resized image from the attached
            wrapper's 'matting' / 'face_parsing' callables (all ones for the face mask with its `cloth`), or both from
            refine_masks=img -> (mask, face_mask); eager, third-party nets -> Stage2.refine_frames, a captured graph with
            use_graphs, whose last launch (emo_stage2_head_f32) writes the bytes that go to the ring, or the fp32 image that
            paste_back=True pastes (paste_matte is then computed on the refined image, and window sides are held to
            output_size_s2 / 4) or that as_uint8=False yields.  Yielded crops are [b,S2,S2,3].  identities, the pose controls
            and smooth_pose are untouched: refinement starts where the render returns, and every rank refines its own shard.
        frame_format='nv12': the frames are NV12 as video decoders hand them out, uint8 [N, 3H/2, W] (H rows of Y, then H / 2
            rows of interleaved U, V; H and W even; stride 1 along a row and a row pitch >= W, so a [..., :W] view of a padded
            surface is taken as it is), 1.5 bytes per pixel on the bus.  The crop step is then ONE launch
            (emo_yuv420_crop_f32: the bytes under each window converted and resized; no full-frame fp32 picture).
            colorspace 'bt709' | 'bt601' and full_range (False: Y 16 ... 235, chroma 16 ... 240) say how the bytes are read
            and written (include/emo_hip.h has the arithmetic).
        out_format: None = frame_format; 'rgb8' | 'nv12' asks for the other one (crops only: paste_back returns the uploaded
            frames, so its out_format is frame_format).  NV12 crops are uint8 [b, 3S/2, S]: the fp32 image, refined or not,
            through emo_pack_yuv420 (image_size / output_size_s2 must be even); with paste_back the NV12 frames are pasted in
            place (emo_paste_yuv420).  as_uint8=False has no out_format.  Everything else -- upload-ahead, the ring,
            smooth_pose, identities, the rank sharding, the caller's frames untouched -- is as for rgb8.
        faces= instead of windows= (both: ValueError): several faces per frame.  faces[i] = the (x_lo, y_lo, side) of frame i in
            paste order, [] for a frame without a face, over the whole frame stream.  A batch is a run of whole frames with at
            most batch_size faces and at most batch_size frames (frames.face_spans; a frame with more faces: ValueError before
            anything is launched; batches are not padded).  Its frames are uploaded once, ONE crop launch cuts all its faces
            out of them (emo_resize2d_faces_f32 / emo_yuv420_crop_f32), the networks run on one row per face, and with
            paste_back=True ONE launch pastes the faces of each frame in list order, the later one on top
            (emo_paste_faces_rgb8 / emo_paste_yuv420): what is yielded is (first_frame_index, frames), a batch without a
            face its frames as they came.  Without paste_back the crops are yielded as (first_face_index, crops), counted over
            the faces of the whole stream; frames without a face yield nothing.  identities= is then one slot per FACE in
            that order, and mix / target_theta=False work per face.  smooth_pose needs identities= and smooth_per_identity=True
            (ValueError otherwise): every face track is its slot's stream.  Ranks shard by FRAMES and take the faces of their
            frames; for smooth_pose the per-face thetas are gathered (parallel.gather_rows).
        expression: an ExpressionControls, or a mapping with its fields -- what happens to the expression vectors between the
            expression embedder and the render, on the device, one launch per batch (ops.expression_controls; the contract is
            hostglue.expression_controls, the reference has only the override, `custome_target_pose_embed`, infer.py:603-604).
            A row is a frame, or a face with faces=.  relative: source expression + (driver_t - driver_first); gain (a float, or
            one per row): the expression damped or exaggerated about the identity's source expression -- both work about the
            source expression of the row's identity (its bank slot's, or the current identity's: what forward(source_image=) left
            in pred_source_pose_embed; a missing one is a ValueError before anything is launched); offset ([E] or [rows,E]) is
            added; smooth, momentum: the smooth_pose recurrence on the expression; override ([rows,E]) replaces the embedder's
            output, and the embedder is then not run.  Order per batch: theta -> pose controls -> expression embedder or
            override -> expression controls -> render.  relative and smooth are scans over the FRAME ORDER with smooth_pose's
            rules: with identities= every row belongs to its slot's stream (anchor and EMA in the bank, reset by a new
            identity in the slot, drop_identity and reset_expression_state), faces= then needs identities, and without
            identities there is one stream whose state the wrapper carries from call to call.  The result does not depend on
            batch_size, on the chunking or on the number of ranks: on one rank the state is carried from batch to batch, on
            several the expressions of every rank's rows are gathered in row order (parallel.gather_rows) and scanned on every
            rank before the render.  None, or all defaults: no launch, no state touched.
        head_pose: a HeadPoseControls, or a mapping with its fields -- what happens to the (scale, rotation, translation) the
            head-pose regressor returns before theta is formed, on the device, one launch per batch (ops.head_pose_controls; the
            contract is hostglue.head_pose_controls).  frontal is the reference's `normalize` and rotation_offset its delta_yaw /
            delta_pitch (expression_embedder.py:302-316) plus roll; relative: source pose + (driver_t - driver_first); gain (a
            float, or one per row): rotation and translation damped or exaggerated about the identity's source pose -- both work
            about the source (scale, rotation, translation) of the row's identity (its bank slot's, or the current identity's,
            pred_source_srt: what the regressor, or a custome_source_theta_embed given as the triple, left behind; a missing one
            is a ValueError before anything is launched, as are frontal with relative and target_theta=False);
            translation_offset is added, zoom multiplies the scale.  Order per batch: regressor -> head-pose controls -> mix,
            smooth_pose on the edited theta -> expression -> render; pred_target_theta / pred_target_srt are what was rendered
            with.  With an active edit the expression embedder is handed the regressor's OWN theta of the row, not the edited
            one: it aligns the driver's crop by that theta, and the driver's face is where the driver's face is; without the
            keyword it gets the mixed / smoothed theta as before.  relative follows the FRAME ORDER with smooth_pose's rules:
            with identities= every row belongs to its slot's stream (the anchor in the bank, restarted by a new identity in the
            slot, drop_identity and reset_pose_state), faces= then needs identities, and without identities there is one stream
            whose anchor the wrapper carries from call to call (restarted by a new source and reset_pose_state).  The result does
            not depend on batch_size, on the chunking or on the number of ranks: on one rank the anchor is carried on the device
            from batch to batch, on several the regressed rows of every rank are gathered in row order (parallel.gather_rows)
            and edited on every rank in the pass in front of the loop that smooth_pose has; without relative the edit is per row
            and needs no gather.  None, or all defaults: no launch, no state touched, the frames bit-identical.
        boxes, tracking: face boxes in place of windows= / faces= (with either: ValueError) -- the crop window arithmetic of
            crop_image (notebooks/infer.py:301-352: box -> centre and size, `scale`, the use_smoothed_crop EMA, fixed_bounding_box,
            remove_overflow) on the device, so that a detector's boxes need not come to the host and the windows of a stream need
            not be known before its first frame is rendered.  boxes: float32 / float64 [N,4], host or device, or an iterable that
            yields one such tensor per chunk of an iterable `frames`, consumed in lockstep (one that ends before the frames do:
            ValueError).  tracking: a CropTracking or a mapping with its fields (smooth, momentum, fixed, scale, box_format
            'xyxy' | 'relative', missing 'skip' | 'hold'); boxes alone is the reference's per-frame window
            (use_smoothed_crop=False).  Per chunk, in front of the batch loop, ONE launch over all rows of the chunk on every rank
            (ops.crop_track, bit for bit hostglue.crop_track; the boxes are inputs every rank has: no gather) forms a crop and a
            paste window per row; the batches slice those device tensors, the crop reads `crop`, paste_back=True pastes at
            `paste`.  The tracker's state is carried on the device from chunk to chunk and from call to call (reset_crop_state,
            forward(reset_tracking=True)); the result does not depend on batch_size, the chunking or the number of ranks.  A row
            whose box is missing (not finite, or beyond 2^30) or whose window does not fit its frame -- with paste_back, is
            smaller than a quarter of the pasted image -- is absent: paste_back returns its frame byte for byte as it went in;
            without paste_back it is still rendered (fixed batch shapes, graphs replay), from the centred square of its frame (or
            with missing='hold' from the track's last window).  Its pose still enters smooth_pose and the relative controls
            unless tracking follow_tracks=True keeps it out (below).  tracked_windows is left as (the paste windows of the chunk
            last tracked, int32 [rows,4] on the device, side 0 = absent; the index of its first row).
            boxes [N,P,4]: P fixed tracks per frame on the faces= path -- rows frame-major, track p is tracker stream p (the
            tracker is made anew when P changes), P <= batch_size, identities= one slot per row, and faces=' rules for smooth_pose
            and the relative controls.  Not here: enrol_identities, paste_back() (it takes device windows already), running a
            detector, and device tensors as windows= (the rgb8 crop kernel trusts its windows; only the tracker's own test makes
            device windows safe to read).
        detections: a detector's output as it comes, in place of boxes= (with boxes=, windows= or faces=: ValueError) -- float32 /
            float64 [N,D,4], host or device, or an iterable of one such tensor per chunk in lockstep: up to D <= 32 boxes per frame
            in NO stable order, a frame with fewer padded with NaN rows.  tracking= must say tracks=P, the number of track slots
            per frame (P <= min(16, batch_size)), and may say min_iou and max_missed.  Per chunk, in front of the tracker's
            launch, ONE more launch on every rank (ops.track_assign, bit for bit hostglue.track_assign: greedy IoU association,
            one wave, the frames in order; no gather) orders the detections into boxes [n,P,4] and a restart flag per row, and
            from there on it is the boxes [N,P,4] path above with ops.crop_track(restart=): rows frame-major, identities= one
            slot per row -- track p is rendered as the identity given for column p -- and faces=' rules for smooth_pose and the
            relative controls.  A new face is born into the lowest free slot and starts the crop EMA at its own box; a track
            without a detection for more than max_missed frames dies, is no longer held by missing='hold', and frees its slot.
            The tracks are carried on the device from chunk to chunk and call to call like the tracker's state, and freed with
            it (reset_crop_state, forward(reset_tracking=True)); the result does not depend on batch_size, the chunking or the
            number of ranks.  tracked_assignment is left as (track_of int32 [n,D]: the track of every detection of the chunk
            last tracked or -1; restart int32 [n,P]), beside tracked_windows.  A row without a face is still rendered, as
            above, and not pasted, unless tracking skip_absent=True leaves it out (below).  Not done: animate_streams keeps one
            track per stream and takes no detections=.  Without the keyword nothing of this is launched.
            tracking follow_tracks=True (with boxes= or detections=): the per-identity control streams -- the smooth_pose EMA, the
            expression controls' relative anchor and EMA, the head-pose controls' relative anchor -- follow the tracks.  Per chunk,
            from what the tracker's launch returned and without a host synchronisation, `present` = the row's paste window has a
            side (a face of its own, or a held window under missing='hold') is formed on the device, and with detections=
            `restart` is track_assign's flag of the row (boxes= has no births: none).  Every launch of the three controls takes
            the slices of both for its rows -- the batches of one rank, the per-chunk passes over all rows on several (every rank
            tracks the whole chunk, so nothing more is gathered) -- through ops.theta_ema_scan / expression_controls /
            head_pose_controls(restart=, present=): emo_*_tracks_f32, bit for bit hostglue.ema_scan_tracks and
            hostglue.expression_controls / head_pose_controls(restart=, present=).  A row walks the stream it walks without the
            field (its identity's bank stream, or the single stream): a birth or a death in its column first restarts that stream,
            so a new face is not smoothed towards the last one's pose nor measured from its first frame; a row without a face is
            rendered from a copy of the stream's state (its own anchor, the start of its own EMA where the stream has none) and
            leaves the stream as it was, so a dropout neither drags the EMA nor becomes the anchor.  mix has no state and stays.
            The result does not depend on batch_size, the chunking or the number of ranks.  tracked_present is left as (present
            int32 [rows] on the device, the index of its first row), beside tracked_windows: a caller can drop the crops of rows
            without a face by it.  Where no control that carries state is active no control launch changes.  Not done:
            animate_streams (ValueError).
            tracking skip_absent=True (with boxes [N,P,4] or detections=; boxes [N,4]: ValueError, pass [N,1,4]): a row without a
            face is not cropped, not embedded, not rendered, not refined and not returned.  Per chunk, behind the tracker's
            launch, ONE more launch over all rows of the chunk on every rank (ops.present_rows, bit for bit
            hostglue.present_rows: a stable compaction in one block) puts the present rows and their windows first, and the
            number of faces of every frame is copied to the host: the ONE host wait per chunk the field adds.  From there the
            call is the faces= call on those windows: a batch is a run of whole frames with at most batch_size present rows and at
            most batch_size frames (frames.face_spans on the counts; batch shapes vary with them, and each shape that recurs is
            captured as a graph of its own), the crop launch, the networks and the paste see kept rows only, the identities are
            identities[row_of].  With paste_back=True what is yielded is (first_frame_index, frames), a batch without a face its
            frames as they came; without it (the index of the batch's first kept row, counted over the kept rows of the call, the
            crops of the kept rows only).  The controls still run over ALL rows of a batch's frames (of the chunk's, in the passes
            over several ranks, which gather the kept rows of every rank): the kept rows are scattered into zeros by row_of, the
            launch is the one of the call that skips nothing -- per-row values (gain, offset, override ...) and the row masks
            stay indexed by the full rows -- and the kept rows of its result are gathered back.  Under follow_tracks an absent row
            neither reads nor writes a stream, so the kept rows and the streams' state after the call are those of the call that
            skips nothing; a control that carries state (smooth_pose, expression relative / smooth, head_pose relative) therefore
            needs follow_tracks=True beside it (ValueError), as_uint8=False is not served (ValueError), and where tracks can
            restart a batch without a face still launches those controls, over zeros, so that a death in it clears its stream.
            Ranks shard by frames; the result does not depend on batch_size, the chunking or the number of ranks.  tracked_rows
            is left as (row_of int32 [T] on the device: the row of the chunk that each kept row is; first: the kept rows in
            front of every frame of the chunk, a host list of n + 1; the index of the chunk's first row); tracked_windows,
            tracked_present and tracked_assignment stay in the full row space.  Not done: animate_streams (ValueError),
            enrol_identities, sharding the ranks by kept rows, padding the batches to a few fixed shapes, hiding the host wait
            behind a tracker stream of its own."""
        if isinstance(frames, torch.Tensor):
            frames_mod.check_frames(frames, frame_format)
        n_rows, counts = frames.shape[0] if isinstance(frames, torch.Tensor) else None, None
        track = control_streams.crop_plan(boxes, tracking, n_rows, 'windows' if windows is not None else 'faces' if faces is not None
                                          else None, batch_size, self.momentum, self.device, detections=detections)
        if track is not None and track.tracks is not None:
            wins = None
            if smooth_pose and (identities is None or not smooth_per_identity):
                raise ValueError("smooth_pose=True with boxes [N,P,4] / detections= smooths every face track as its identity's stream: pass identities= "
                                 "(one slot per row) and smooth_per_identity=True")
            n_rows = None if n_rows is None else n_rows * track.tracks          # identities: one slot per row
            if identities is not None and n_rows is not None and len(identities) != n_rows:
                raise ValueError(f"identities has {len(identities)} entries for {n_rows} rows: one slot per track of every frame")
        elif faces is not None:
            if windows is not None:
                raise ValueError("faces= (a list of windows per frame) and windows= (one per frame) are mutually exclusive")
            wins, counts = frames_mod.flatten_faces(faces)
            if n_rows is not None and len(counts) != n_rows:
                raise ValueError(f"faces has {len(counts)} entries for {n_rows} frames")
            if max(counts, default=0) > batch_size:
                raise ValueError(f"a frame has {max(counts)} faces: more than batch_size={batch_size}")
            if smooth_pose and (identities is None or not smooth_per_identity):
                raise ValueError("smooth_pose=True with faces= smooths every face track as its identity's stream: pass identities= "
                                 "(one slot per face) and smooth_per_identity=True")
            n_rows = len(wins)                                                   # identities: one slot per face
            if identities is not None and len(identities) != n_rows:
                raise ValueError(f"identities has {len(identities)} entries for {n_rows} faces: one slot per face")
        else:
            wins = None if windows is None else frames_mod.square_windows(windows)
        plan = self._video_plan(n_rows=n_rows, wins=wins, identities=identities, batch_size=batch_size, ring=ring, to_host=to_host,
                                smooth_pose=smooth_pose, smooth_per_identity=smooth_per_identity, mix=mix, mix_old=mix_old,
                                target_theta=target_theta, paste_back=paste_back, feather=feather, paste_matte=paste_matte,
                                as_uint8=as_uint8, refine=refine, refine_masks=refine_masks, frame_format=frame_format,
                                out_format=out_format, colorspace=colorspace, full_range=full_range, expression=expression,
                                faces=faces is not None or track is not None and track.tracks is not None, head_pose=head_pose, track=track)
        yield from self._animate_clip(frames, wins, counts, plan)

    def _video_plan(self, *, n_rows, wins, identities, batch_size, ring, to_host, smooth_pose, smooth_per_identity, mix, mix_old,
                    target_theta, paste_back, feather, paste_matte, as_uint8, refine, refine_masks, frame_format, out_format,
                    colorspace, full_range, arena=False, expression=None, where='animate_frames', faces=False, head_pose=None,
                    track=None):
        """The checks of the keywords animate_frames() and animate_streams() share, before anything is launched, and what their
        loops need beside the frames: wins = the (x0, y0, s, s) of every row of the call (None: whole frames), n_rows their
        number where it is known.  -> masks_of, ids (_preflight), matte_fn (_paste_matte), out_kind (_render's `out`), fmt =
        (frame_format, colorspace, full_range), ring = the pinned ring (None without to_host; with `arena` and paste_back a
        frames.ArenaRing), upload_stream, ex, hp = the expression and the head-pose controls (_control_plans;
        None: none), track = the crop tracking of boxes= (control_streams.crop_plan; None: none -- it forms the windows on the
        device, and `wins` is then None) with min_side = the smallest side it lets through (a quarter of the pasted image, or 2),
        row_masks = None until _track fills it per chunk under tracking follow_tracks=True, and the loop's keywords as they came."""
        frames_mod.check_format(frame_format, colorspace)
        if out_format is not None:
            frames_mod.check_format(out_format, colorspace, "out_format")
            if not as_uint8:
                raise ValueError("as_uint8=False yields the fp32 device image: it has no out_format")
        out_format = out_format or frame_format
        if paste_back and out_format != frame_format:
            raise ValueError(f"paste_back=True returns the uploaded {frame_format} frames: out_format={out_format!r} is not possible")
        if not as_uint8 and (to_host or paste_back):
            raise ValueError("as_uint8=False yields the fp32 device image: it needs to_host=False and paste_back=False")
        masks_of, ids = self._preflight(n_rows, identities, mix, target_theta, smooth_pose, smooth_per_identity, refine, refine_masks)
        matte_fn, min_side = None, 2
        if paste_back:
            if wins is None and track is None:
                raise ValueError("paste_back=True needs windows= or faces=: (x_lo, y_lo, side) says where each rendered crop goes")
            if not 0.0 <= float(feather) <= 0.5:
                raise ValueError(f"feather {feather} is a fraction of the window side: 0 ... 0.5")
            matte_fn = self._paste_matte(paste_matte, 'paste_matte=True')
            S_out = self.cfg["image_size"] if masks_of is None else self._stage2.cfg["output_size_s2"]
            min_side = max(min_side, -(-S_out // 4))
            if wins is not None and any(4 * w[2] < S_out for w in wins):
                raise ValueError(f"a paste window is smaller than a quarter of the {S_out}-pixel image: downscaling "
                                 f"stops at image_size / 4")
        if out_format != "rgb8" and as_uint8 and not paste_back:
            self._yuv420_size(masks_of, out_format)
        out_kind = "f32" if paste_back or not as_uint8 else ("u8" if out_format == "rgb8" else out_format)
        ex, hp = self._control_plans(expression, head_pose, n_rows, ids, where, target_theta, faces)
        if track is not None and track.skip_absent:
            if not as_uint8:
                raise ValueError("tracking skip_absent=True yields the rows that have a face: as_uint8=False (the render's own output "
                                 "buffer, one row per slot) is not served")
            stateful = [name for name, on in (("smooth_pose", smooth_pose), ("expression relative / smooth", ex is not None and ex.scan),
                                              ("head_pose relative", hp is not None and hp.relative)) if on]
            if stateful and not track.follow_tracks:
                raise ValueError(f"tracking skip_absent=True with {stateful[0]}: without follow_tracks=True a row without a face is a "
                                 f"step of its identity's stream and cannot be left out: pass follow_tracks=True as well")
        host_ring = None if not to_host else (frames_mod.ArenaRing(self.device, ring) if arena and paste_back
                                              else frames_mod.HostRing(self.device, ring, batch_size))
        return Namespace(masks_of=masks_of, ids=ids, matte_fn=matte_fn, out_kind=out_kind, fmt=(frame_format, colorspace, bool(full_range)),
                         feather=feather, paste_back=paste_back, ring=host_ring, upload_stream=torch.cuda.Stream(device=self.device),
                         batch_size=batch_size, smooth_pose=smooth_pose, mix=mix, mix_old=mix_old, target_theta=target_theta, ex=ex,
                         hp=hp, track=track, min_side=min_side, row_masks=None)

    def _control(self, at, fn, *inputs):
        """One launch of a control over the rows `at` (a frames.RowsAt): fn(*inputs over the full rows, their slots, the first one's
        index in the call) -> a tensor or a tuple of tensors over those rows.  at.at None: the inputs [m, ...] ARE the full rows and go
        to fn as they came.  Else (tracking skip_absent=True) they are the kept rows: they are scattered into zeros [at.n, ...] by at.at
        (an absent row reads zeros), the launch is the one of the call that skips nothing -- per-row values and row masks indexed by the
        full rows -- and the kept rows of its result come back.  No kept row at all: the launch over zeros, nothing comes back."""
        if at.at is None:
            return fn(*inputs, at.slots, at.r0)
        wide = [torch.zeros((at.n,) + tuple(t.shape[1:]), device=self.device, dtype=t.dtype).index_copy_(0, at.at, t)
                for t in (t.to(self.device).float() for t in inputs)]
        out = fn(*wide, at.slots, at.r0)
        return tuple(t.index_select(0, at.at) for t in out) if isinstance(out, tuple) else out.index_select(0, at.at)

    def _expression_width(self):
        """E of the expression vectors: the bank's rows' where it has some, else the configuration's"""
        return self._bank_expr.shape[1] if self._bank_expr is not None else self.cfg["lpe_output_channels_expression"]

    def _override_rows(self, ex, at):
        """the expression override of the rows `at`: read over their full rows, the kept ones selected where rows were left out"""
        rows = control_streams.rows_of(ex.override, at.r0, at.n, 'expression override')
        return rows if at.at is None else rows.index_select(0, at.at)

    def _batch_theta(self, crops, at, plan, edit=True, mix=True, smooth=None):
        """The front of a driver batch of the video paths, crops [m,3,S,S] = the rows `at` of the call (a frames.RowsAt) -> (theta,
        align): the head pose the regressor finds, edited per row by the head-pose controls (plan.hp, over the full rows: _control) and
        then mixed (mix has neither state nor per-row values: on the rows themselves), and what the expression embedder aligns the
        crops by -- under an active head-pose edit the regressor's OWN theta of the rows, else None = the theta the batch is rendered
        with.  Either may be the regressor's output buffer: a caller that holds it past the batch clones it.  pred_target_srt is
        left as the edit of the batch's rows.
        edit=False: a pass that gathers the rows of every rank edits them, and in theta's place come the regressed (scale, rotation,
        translation) as [m,9] rows.  mix=False: the caller mixes, once over its rows of the chunk.  smooth: None = mix alone, and
        only where plan.mix asks for it (a clip); a bool = mix and the one-pass smooth_pose of the batch's rows (streams)."""
        theta, *srt = self._head_pose(crops)
        align = None
        if plan.hp is not None:
            align = theta
            if not edit:
                theta = self._srt9(srt)
            else:
                edited, theta = self._control(at, lambda a, b, c, slots, r: self._head_pose_controls((a, b, c), slots, plan.hp, r,
                                                                                                     plan.row_masks), *srt)
                self.pred_target_srt = tuple(edited[:, i:i + 3] for i in (0, 3, 6))
        if mix and (plan.mix or smooth is not None):
            theta = self._pose_controls(theta, at.ident, plan.mix, plan.mix_old, bool(smooth), at.r0, plan.row_masks)
        return theta, align

    def _batch_expression(self, crops, theta, align):
        """the expression embedder on a driver batch: its crops aligned by `align` (_batch_theta), or by the theta it is rendered with"""
        return self._expression(crops, theta if align is None else align, 'a driver call')[0]

    def _drive_crops(self, crops, at, plan, theta=None, smooth=None, pose=None, align=None):
        """The sequence of one driver batch of the video paths, crops [m,3,S,S] = the rows `at` of the call (a frames.RowsAt: the
        controls' per-row values and slots) -> (the rendered batch as plan.out_kind says, its paste matte or None): head pose ->
        head-pose controls -> pose controls (_batch_theta) -> expression embedder (or the override) -> expression controls -> render
        -> matte, in forward()'s order.  theta, align: the batch's thetas and what the embedder aligns by where a pass in front of
        the loop has formed them (the passes of a clip that walk the rows of several ranks); pose: its controlled expressions
        likewise.  smooth: _batch_theta's."""
        if theta is None:
            theta, align = self._batch_theta(crops, at, plan, smooth=smooth)
        self.pred_target_theta = theta                                           # (as forward() leaves it: infer.py:584)
        ex = plan.ex
        if pose is None:
            pose = self._override_rows(ex, at) if ex is not None and ex.override is not None else self._batch_expression(crops, theta, align)
            if ex is not None:
                pose = self._control(at, lambda v, slots, r: self._expression_controls(v, slots, ex, r, plan.row_masks), pose)
        out = self._render(pose, theta, at.ident, plan.target_theta, plan.masks_of, plan.out_kind, plan.fmt[1:])
        return out, (None if plan.matte_fn is None else plan.matte_fn(out).float().contiguous())

    def _track(self, states, boxes, stream_of, sizes, plan, row0, restart=None):
        """boxes= -> windows: ONE launch over the rows `boxes` [m,4] in frame order (ops.crop_track, bit for bit hostglue.crop_track),
        row i on track stream_of[i] of `states` (a control_streams.CropStates; None: the one track) in a frame of sizes = (W, H), or
        one (W, H) per row, with the settings of plan.track -> (crop, paste) windows of the rows as ops.DeviceWindows.
        tracked_windows = (paste [m,4], row0 = the first row's index in the call).  restart [m] int32 or None: the rows at which
        their track begins again (ops.track_assign's).  With tracking follow_tracks=True tracked_present = (present int32 [m]: the
        row's paste window has a side, row0) and plan.row_masks = (restart, present, row0), which the control streams of the chunk's
        batches take (control_streams.row_masks)."""
        t = plan.track
        more = {} if restart is None else dict(restart=restart)
        crop, paste, _ = ops.crop_track(boxes, stream_of, sizes, *states.arrays(), momentum=t.momentum, smooth=t.smooth, fixed=t.fixed,
                                        scale=t.scale, box_format=t.box_format, missing=t.missing, min_side=plan.min_side, **more)
        self.tracked_windows = (paste, row0)
        if t.follow_tracks:
            # a row has a face where the tracker gave it a paste window with a side: one comparison on the device per chunk
            self.tracked_present = ((paste[:, 2] > 0).to(torch.int32), row0)
            plan.row_masks = (restart, self.tracked_present[0], row0)
        return ops.DeviceWindows(crop), ops.DeviceWindows(paste)

    def _track_chunk(self, plan, n, base, frame_hw, row0):
        """boxes= for the n frames of a chunk (the frames base ... of the call, H x W = frame_hw): their boxes from the feed, tracked
        over all their rows in frame order (_track) with the tracks' state carried in _crop_streams.  Track p of boxes [N,P,4] is
        tracker stream p; the store is made anew when the number of tracks changes.  detections=: the feed hands out the chunk's
        detections [n,D,4], which ONE launch in front (ops.track_assign, the tracks carried in _track_states and made anew with
        the tracker's store) orders into boxes [n,P,4] and the rows' restart flags; tracked_assignment = (track_of, restart)."""
        if n == 0:
            return (ops.DeviceWindows(torch.empty((0, 4), dtype=torch.int32, device=self.device)),) * 2
        t = plan.track
        boxes = t.feed.take(n, base)
        K = t.tracks or 1
        if self._crop_streams is None or self._crop_streams.K != K:
            self._crop_streams = control_streams.CropStates(K, self.device)
            self._track_states = None
        restart = None
        if t.detections is not None:
            if self._track_states is None:
                self._track_states = control_streams.TrackStates(1, K, self.device)
            ts = self._track_states
            boxes, restart, track_of = ops.track_assign(boxes, None, ts.ref, ts.age, t.min_iou, t.max_missed, t.box_format)
            self.tracked_assignment = (track_of, restart)
            restart = restart.reshape(-1)
        stream_of = None if t.tracks is None else torch.arange(K, dtype=torch.int32).repeat(n).to(self.device)
        return self._track(self._crop_streams, boxes.reshape(-1, 4), stream_of, (frame_hw[1], frame_hw[0]), plan, row0, restart)

    def _animate_clip(self, frames, wins, counts, plan):
        """animate_frames behind its checks.  A row of everything between the crop and the paste is a face: wins = the
        (x0, y0, s, s) of every row of the stream in frame order, counts[i] = the faces of frame i, plan.ids = the slot of every
        row (host tensor) or None.  counts=None is windows= / whole frames: one row per frame (wins None: the whole frame), the
        per-frame entry points (frame_of=None) and the single-stream smooth_pose.  Per chunk the frames are sharded across the
        ranks; a batch is a span of whole frames (frames.face_spans).  With plan.track (boxes=) wins is None: the windows of a
        chunk are formed on the device in front of its batches (_track_chunk), P rows per frame where the boxes are [N,P,4].
        The row arithmetic of a chunk -- which rows a span of frames holds, the rank's shard, its batches -- is one
        frames.ChunkRows, `rows`; a batch is handed rows.where(b0, b1), a frames.RowsAt, and every control is launched through
        _control with it.
        A chunk is rendered in up to three passes over the spans of the rank's frames, each through `walk`: the head-pose pass
        (smooth_pose, or a relative head pose on several ranks) and the expression pass (relative / smooth on several ranks) form
        the thetas and the expressions that follow the frame order across the ranks (`scan`), the render pass drives the batches.
        tracking skip_absent=True: the rows of the loop are the KEPT rows, those the tracker found a face for.  The chunk is
        tracked first, ONE launch over all its rows on every rank puts the present rows and their windows first
        (ops.present_rows), and the number of faces of every frame is copied to the host -- the one host wait per chunk the field
        adds, on every rank.  From there per[i] is that number, exactly as faces= counts its faces: the spans hold at most
        batch_size kept rows, the crop, the networks, the paste and what is yielded see kept rows only, and the identities are
        ids[row_of].  The controls alone still run over the full rows of a span's frames (the RowsAt then says where the kept rows
        lie among them, and _control scatters and gathers; over the chunk's in `scan`), and where a track can restart a span
        without a kept row still launches the controls that carry state -- the same _control, with no kept row: over zeros -- so a
        death in it clears its stream as it does in the call that skips nothing.  tracked_rows = (row_of [T], first,
        the chunk's first full row); tracked_windows, tracked_present and tracked_assignment stay in the full row space."""
        S, ids, paste_back, ex, hp = self.cfg["image_size"], plan.ids, plan.paste_back, plan.ex, plan.hp
        P = None if plan.track is None else plan.track.tracks
        skip = plan.track is not None and plan.track.skip_absent
        base = row0 = full0 = 0                                                  # (full0: the chunk's first full row, under skip)
        for chunk in [frames] if isinstance(frames, torch.Tensor) else frames:
            frames_mod.check_frames(chunk, plan.fmt[0])
            n = chunk.shape[0]
            if counts is not None and base + n > len(counts):
                raise ValueError(f"faces has {len(counts)} entries, the frames run past it")
            # which rows a span of frames holds: per[i] = the rows of the chunk's frame i -- the faces of faces=, the P tracks of boxes
            # [N,P,4], or None for one row per frame and the per-frame entry points (windows=, boxes [N,4], whole frames)
            per = [P] * n if P is not None else None if counts is None else counts[base:base + n]
            if counts is None and ids is not None and (full0 if skip else row0) + n * (P or 1) > ids.shape[0]:
                raise ValueError(f"identities has {ids.shape[0]} entries, the frames run past it")
            tracked, row_of = None, torch.empty((0,), dtype=torch.int64, device=self.device) if skip else None
            if plan.track is not None:
                # every rank tracks the whole chunk (the boxes are inputs every rank has), then slices its batches' windows
                tracked = self._track_chunk(plan, n, base, frames_mod.frame_size(chunk, plan.fmt[0]) if n else None, full0 if skip else row0)
            if skip and n:
                count, _, row_of, *tracked = ops.present_rows(tracked[0].tensor, tracked[1].tensor, n, P)
                per = count.tolist()                                             # (the host wait of the chunk)
                self.tracked_rows = (row_of[:sum(per)], frames_mod.face_offsets(per), full0)
                row_of = self.tracked_rows[0].long()
                tracked = [ops.DeviceWindows(w) for w in tracked]                # (the kept rows' windows, compacted)
            rows =frames_mod.ChunkRows(n, per, self.rank, self.world, plan.batch_size, row0, ids, self.device, P, full0, row_of)
            crop_w = paste_w = None if wins is None else wins[rows.m_lo:rows.m_hi]
            if tracked is not None:
                crop_w, paste_w = (rows.shard(w) for w in tracked)
            # a track that restarts does so whether or not its row is kept: under skip, with restart flags, the spans without a
            # kept row still launch the controls that carry state from batch to batch on this rank
            restarts = skip and plan.row_masks is not None and plan.row_masks[0] is not None
            # crops stay resident from one pass to the next (3 MB per frame at 512^2) while the rank's rows of the chunk fit the budget
            keep = (rows.m_hi - rows.m_lo) * 3 * S * S * 4 <= _SMOOTH_KEEP_BYTES
            kept, thetas, aligns, poses = {}, {}, {}, None
            # the two controls as _control launches them: fn(the full rows, their slots, the first one's index in the call)
            hp_fn = lambda a, b, c, slots, r: self._head_pose_controls((a, b, c), slots, hp, r, plan.row_masks)
            ex_fn = lambda v, slots, r: self._expression_controls(v, slots, ex, r, plan.row_masks)

            def walk(last=False):
                """(b0, b1, crops, uploaded frames or None) for every span a pass needs: the crops an earlier pass kept, or a fresh
                upload (span i + 1 beside the compute of span i: frames.uploaded) and ONE crop launch.  A span without a face is not
                uploaded for crops, a kept span not again -- unless its frames are what the render is pasted into (last, with
                paste_back: the crops were kept, not the frames, 6 MB at 1080p; a span without a face then comes with crops None).
                The last pass lets go of what was kept."""
                pasted = last and paste_back
                need = rows.spans if pasted or restarts else rows.with_rows     # (restarts: walk's callers launch `absent`)
                fresh = frames_mod.uploaded(chunk, [sp for sp in need if pasted or sp[0] not in kept and sp in rows.with_rows], self.device,
                                            plan.upload_stream)
                for b0, b1 in need:
                    crops, u8 = kept.pop(b0, None) if last else kept.get(b0), None
                    if pasted or crops is None and (b0, b1) in rows.with_rows:
                        f0, f1, u8 = next(fresh)
                        assert (f0, f1) == (b0, b1)
                    if crops is None and (b0, b1) in rows.with_rows:
                        crops = frames_mod.crops_of(u8, S, rows.part(crop_w, b0, b1), *plan.fmt, frame_of=rows.frame_of(b0, b1))
                        if keep and not last:
                            kept[b0] = crops
                    yield b0, b1, crops, u8

            def scan(fn, local=None, every=None):
                """A control that walks the rows of every rank in frame order: the rank's rows `local` of the chunk are gathered in
                row order on every rank (every=: a function of the chunk's RowsAt that returns rows every rank has already),
                fn runs over the whole chunk on every rank (_control) -- so the streams' state is the same everywhere, whichever
                rank formed a row -- and the rank's own rows of the result come back."""
                at = rows.where_chunk()
                every = every(at) if every is not None else local if rows.counts is None else \
                    parallel.gather_rows(local, rows.counts, self.rank, self.world)
                return rows.shard(self._control(at, fn, every))

            def absent(b0, b1, head, expression):
                """skip with restart flags: the frames [b0, b1) hold no kept row, and the controls that carry state from batch to
                batch on this rank are still launched over their rows -- _control with no kept row: over zeros -- so that a restart
                in them reaches its stream.  (pred_target_srt is then the edit of those full rows.)"""
                at = rows.where(b0, b1)
                if head and hp is not None and hp.relative and not gather_srt:
                    self._control(at, hp_fn, *(torch.empty((0, 3), device=self.device) for _ in range(3)))
                if expression and ex is not None and ex.scan and self.world == 1:
                    self._control(at, ex_fn, torch.empty((0, self._expression_width()), device=self.device))

            def front(b0, b1, crops, **kw):
                """_batch_theta on a span in a pass in front of the render; what the embedder aligns by is kept for the passes behind"""
                theta, align = self._batch_theta(crops, rows.where(b0, b1), plan, **kw)
                if align is not None:
                    aligns[b0] = align.clone()
                return theta, align

            # a relative head pose walks the rows of every rank: their regressed (scale, rotation, translation) are gathered and edited
            # on every rank, so the anchor is the stream's first row whichever rank regressed it
            gather_srt = hp is not None and hp.relative and self.world > 1
            if plan.smooth_pose or gather_srt:
                local = []
                for b0, b1, crops, _ in walk():
                    if crops is None:
                        absent(b0, b1, True, False)
                        continue
                    theta, align = front(b0, b1, crops, edit=not gather_srt, mix=False)
                    local.append(theta.clone() if align is None else theta)
                local = torch.cat(local) if local else torch.empty((0, 9) if gather_srt else (0, 4, 4), device=self.device)
                if gather_srt:
                    local = scan(lambda every, slots, r: hp_fn(*(every[:, i:i + 3].contiguous() for i in (0, 3, 6)), slots, r)[1], local)
                if plan.mix:
                    local = self._pose_controls(local, rows.ident, True, plan.mix_old, False)
                if plan.smooth_pose:
                    local = scan(lambda every, slots, r: self._pose_controls(every, slots, False, plan.mix_old, True, r, plan.row_masks),
                                 local)
                thetas = {b0: rows.part(local, b0, b1) for b0, b1 in rows.with_rows}
            if ex is not None and ex.scan and self.world > 1:
                # relative / smooth walk the rows of every rank: the expressions of the rank's rows, or the override's, which every rank has
                if ex.override is not None:
                    poses = scan(ex_fn, every=lambda at: self._override_rows(ex, at))
                else:
                    local = []
                    for b0, b1, crops, _ in walk():
                        if crops is None:                                        # (restarts: nothing here carries state on this rank alone)
                            continue
                        if b0 not in thetas:
                            thetas[b0] = front(b0, b1, crops)[0].clone()
                        local.append(self._batch_expression(crops, thetas[b0], aligns.get(b0)).float().clone())
                    # (a rank without a row still joins the gather)
                    poses = scan(ex_fn, torch.cat(local) if local else torch.empty((0, self._expression_width()), device=self.device))
            for b0, b1, crops, u8 in walk(last=True):
                m0 = rows.rows(b0, b1)[0]
                if crops is None and restarts:                                   # (the head pose: unless a pass in front has walked it)
                    absent(b0, b1, not plan.smooth_pose, True)
                    if not paste_back:
                        continue
                if crops is None:                                                # (paste_back: frames without a face, as they came)
                    out = u8.clone() if chunk.is_cuda else u8
                else:
                    out, m = self._drive_crops(crops, rows.where(b0, b1), plan, thetas.pop(b0, None), pose=rows.part(poses, b0, b1),
                                               align=aligns.pop(b0, None))
                    if paste_back:
                        full = u8.clone() if chunk.is_cuda else u8               # (a host chunk's upload is this span's own)
                        out = frames_mod.paste_into(full, out, rows.part(paste_w, b0, b1), plan.feather, m, *plan.fmt,
                                                    frame_of=rows.frame_of(b0, b1))
                index = base + b0 if paste_back else m0
                if plan.ring is not None:
                    yield from plan.ring.push(index, out)
                else:
                    yield index, out
            base, row0, full0 = base + n, rows.r1, full0 + (n * P if skip else 0)
        if plan.ring is not None:
            yield from plan.ring.drain()

    def animate_streams(self, streams, batch_size=16, ring=3, to_host=True, smooth_pose=False, mix=False, mix_old=True,
                        target_theta=True, paste_back=False, feather=0.0625, paste_matte=None, as_uint8=True, refine=False,
                        refine_masks=None, frame_format="rgb8", out_format=None, colorspace="bt709", full_range=False,
                        expression=None, head_pose=None, tracking=None):
        """Several video streams of DIFFERENT frame sizes served by one driver batch: animate_frames(faces=) with the frames of a
        batch a list instead of one tensor.  Between the crop and the paste everything is one row per face, so only the two ends
        differ: ONE crop launch reads every face of the batch out of its own frame through a frame table
        (ops.crop_faces_mixed: emo_rgb8_faces_ragged_f32 reads the bytes under the windows only, no full-frame fp32 picture;
        emo_yuv420_crop_ragged_f32), then the steps animate_frames runs (_head_pose, _pose_controls, _expression, _render), and
        with paste_back=True ONE paste launch (ops.paste_faces_mixed).
        streams: a list of mappings, one per stream --
            'frames': uint8 [N_s,H_s,W_s,3] (NV12: [N_s,3H_s/2,W_s]) or an iterable of such chunks, host (ideally pinned) or device;
            'windows': one (x_lo, y_lo, side) per frame, or 'faces': a list of them per frame in paste order ([]: no face); their
                length is the stream's number of frames;
            or 'boxes' in place of both (then in every stream): the face box of every frame, float32 / float64 [N_s,4], or an
                iterable of such chunks in lockstep with the stream's frames (the stream's length must be known: its frames or
                its boxes are one tensor) -- animate_frames' boxes=, with tracking= (one per call) saying how they become windows.
                ONE launch per batch forms the batch's windows (ops.crop_track with stream_of = each row's stream and the (W, H)
                of each row's own frame); the trackers' state, one per stream, is the call's own and is carried on the device from
                batch to batch.  Several tracks per stream are out of scope;
            'identities' (optional, then in every stream): one bank slot for the stream, or one per face of the stream;
            'expression' (optional): {'gain': a float or one per face of the stream, 'offset': [E] or one row per face}, in place
                of the call's values for this stream;
            'head_pose' (optional): {'gain', 'zoom': a float or one per face of the stream, 'rotation_offset',
                'translation_offset': [3] or one row per face}, in place of the call's values for this stream.
        head_pose: animate_frames' head-pose controls, here with the flags, a scalar gain / zoom and [3] offsets; relative needs
            identities, every face track is its slot's stream, edited batch by batch in one pass as smooth_pose is.  (With
            per-stream offsets a stream without one is given a zero offset.)
        expression: animate_frames' expression controls, here with the flags, the momentum, a scalar gain and an [E] offset (no
            override); relative and smooth need identities, every face track is its slot's stream, scanned batch by batch in one
            pass as smooth_pose is.  (With per-stream offsets a stream without one is given a zero offset.)
        Order: tick t takes frame t of every stream that still has one, in stream order (frames.interleave).  A batch is a run
        of whole frames of that sequence, taken greedily while it holds at most batch_size faces and at most batch_size frames
        (frames.face_spans; a frame with more faces: ValueError before anything is launched).
        The frames of a batch live in one device byte buffer, each at a 256-byte aligned offset, every host frame uploaded by
        its own asynchronous copy, batch i + 1 before batch i's kernels (frames.uploaded_mixed).  Device frames are read where
        they lie and copied into the arena only to be pasted into: the caller's frames stay untouched.
        smooth_pose needs identities (ValueError otherwise): every face track is its slot's stream (animate_frames'
        smooth_per_identity), scanned batch by batch in one pass -- the slots' states are carried on the device.
        The other keywords and their checks are animate_frames'; there is one frame_format per call.
        Yields, per batch, a list of (stream, frame index in the stream, out): with paste_back the pasted frame [H_s,W_s,3]
        (NV12 [3H_s/2,W_s]) -- with to_host a view of a pinned ring slot that received the whole arena in ONE copy
        (frames.ArenaRing), a frame without a face as it went in; otherwise that frame's crops [faces,S,S,3] (out_format 'nv12':
        [faces,3S/2,S]; as_uint8=False: fp32 [faces,3,S,S]), frames without a face left out.  Everything yielded is valid until
        the generator is resumed.
        The call is rank-local: no collective, no sharding -- each rank serves its own streams."""
        faces, idents, tracks = [], [], []
        tracked = any('boxes' in st for st in streams)
        if tracking is not None and not tracked:
            raise ValueError("tracking= says how a stream's 'boxes' become windows: no stream has any")
        if tracking is not None and control_streams.CropTracking.of(tracking).skip_absent:
            raise ValueError("tracking skip_absent=True is animate_frames': animate_streams renders every row of its streams")
        for k, st in enumerate(streams):
            if tracked:
                if 'boxes' not in st:
                    raise ValueError("'boxes' must be given in every stream or in none")
                n_k = st['frames'].shape[0] if isinstance(st['frames'], torch.Tensor) else \
                    st['boxes'].shape[0] if isinstance(st['boxes'], torch.Tensor) and st['boxes'].dim() else None
                tr = control_streams.crop_plan(st['boxes'], tracking, n_k, next((o for o in ('windows', 'faces') if o in st), None),
                                               batch_size, self.momentum, self.device, f"stream {k}: 'boxes'")
                if tr.tracks is not None:
                    raise ValueError(f"stream {k}: 'boxes' must be [N,4]: several tracks per stream are not served")
                if tr.follow_tracks:
                    raise ValueError("tracking follow_tracks=True is animate_frames': the control streams of animate_streams do not "
                                     "follow its tracks")
                if n_k is None:
                    raise ValueError(f"stream {k}: its length must be known before the first batch: give its frames or its boxes as one tensor")
                tracks.append(tr)
                of_stream = [[(0, 0, 1)]] * n_k                                  # (one face per frame; the windows come from the tracker)
            else:
                if ('windows' in st) == ('faces' in st):
                    raise ValueError(f"stream {k} takes either 'windows' (one per frame) or 'faces' (a list per frame)")
                of_stream = [[w] for w in st['windows']] if 'windows' in st else list(st['faces'])
            flat, counts = frames_mod.flatten_faces(of_stream)
            if isinstance(st['frames'], torch.Tensor):
                frames_mod.check_frames(st['frames'], frame_format)
                if st['frames'].shape[0] != len(counts):
                    raise ValueError(f"stream {k} has {len(counts)} entries of windows / faces for {st['frames'].shape[0]} frames")
            faces.append((flat, counts))
            ids = st.get('identities')
            if ids is not None:
                ids = [int(v) for v in ids] if hasattr(ids, '__len__') else [int(ids)] * len(flat)
                if len(ids) != len(flat):
                    raise ValueError(f"stream {k}: identities has {len(ids)} entries for {len(flat)} faces: one slot, or one per face")
            idents.append(ids)
        if any(i is None for i in idents) and not all(i is None for i in idents):
            raise ValueError("'identities' must be given in every stream or in none")
        if smooth_pose and (not idents or idents[0] is None):
            raise ValueError("smooth_pose=True smooths every face track as its identity's stream: give every stream 'identities'")
        order = frames_mod.interleave([len(counts) for _, counts in faces])
        first = [frames_mod.face_offsets(counts) for _, counts in faces]         # first[s][t] = faces of stream s in front of its frame t
        counts = [faces[s][1][t] for s, t in order]
        spans = frames_mod.face_spans(counts, 0, len(order), batch_size)
        wins = [w for s, t in order for w in faces[s][0][first[s][t]:first[s][t + 1]]]
        identities = None if not idents or idents[0] is None else [i for s, t in order for i in idents[s][first[s][t]:first[s][t + 1]]]
        n_faces, spans_of = [len(flat) for flat, _ in faces], [(s, first[s][t], first[s][t + 1]) for s, t in order]
        expression = control_streams.stream_expression(expression, [st.get('expression') for st in streams], n_faces, spans_of)
        head_pose = control_streams.stream_head_pose(head_pose, [st.get('head_pose') for st in streams], n_faces, spans_of)
        plan = self._video_plan(n_rows=len(wins), wins=None if tracked else wins, identities=identities, batch_size=batch_size, ring=ring,
                                to_host=to_host, smooth_pose=smooth_pose, smooth_per_identity=True, mix=mix, mix_old=mix_old,
                                target_theta=target_theta, paste_back=paste_back, feather=feather, paste_matte=paste_matte,
                                as_uint8=as_uint8, refine=refine, refine_masks=refine_masks, frame_format=frame_format,
                                out_format=out_format, colorspace=colorspace, full_range=full_range, arena=True, expression=expression,
                                where='animate_streams', head_pose=head_pose, track=tracks[0] if tracked else None)
        crop_states = control_streams.CropStates(len(streams), self.device) if tracked else None     # (the call's own)
        S, host_ring = self.cfg["image_size"], plan.ring
        ids_dev = None if plan.ids is None else plan.ids.to(self.device)
        rows = frames_mod.face_offsets(counts)                                   # rows[i] = faces in front of frame i of the order
        todo = [sp for sp in spans if paste_back or rows[sp[0]] < rows[sp[1]]]   # (crops: a batch without a face is not uploaded)

        def frames_of(k, st):
            """the frames of stream k one by one, chunk after chunk"""
            n = 0
            for chunk in [st['frames']] if isinstance(st['frames'], torch.Tensor) else st['frames']:
                frames_mod.check_frames(chunk, frame_format)
                for i in range(chunk.shape[0]):
                    if n == len(faces[k][1]):
                        raise ValueError(f"stream {k}: its windows / faces have {n} entries, the frames run past it")
                    n += 1
                    yield chunk[i]
        readers = [frames_of(k, st) for k, st in enumerate(streams)]

        def boxes_of(k):
            """the boxes of stream k one by one, chunk after chunk"""
            feed = tracks[k].feed
            for chunk in [feed.whole] if feed.whole is not None else feed.chunks:
                if control_streams.check_boxes(chunk, f"stream {k}: a chunk of 'boxes'") is not None:
                    raise ValueError(f"stream {k}: 'boxes' must be [N,4]")
                yield from chunk
        box_readers = [boxes_of(k) for k in range(len(tracks))]

        def batches():
            at = 0
            for b0, b1 in spans:                                                 # (every frame is taken from its stream, in order)
                batch = []
                for s, t in order[b0:b1]:
                    frame = next(readers[s], None)
                    if frame is None:
                        raise ValueError(f"stream {s} has {t} frames, its windows / faces have {len(faces[s][1])} entries")
                    batch.append(frame)
                if at < len(todo) and todo[at] == (b0, b1):
                    at += 1
                    yield batch

        def handed_out(meta, buf):
            """a finished batch -> [(stream, frame index, out)]: the frames of an arena (or of the ring slot that received it),
            or the rows of the crops split by frame"""
            if paste_back:
                shapes = [shape for _, _, shape in meta]
                dtype = ops.yuv420_dtype(frame_format)
                views = frames_mod.arena_views(buf, shapes, frames_mod.arena_layout(shapes, 2 if dtype == torch.uint16 else 1)[0], dtype)
                return [(s, t, v) for (s, t, _), v in zip(meta, views)]
            out, m = [], 0
            for s, t, c in meta:
                if c:
                    out.append((s, t, buf[m:m + c]))
                m += c
            return out

        fresh = frames_mod.uploaded_mixed(batches(), self.device, plan.upload_stream, paste_back)
        for b0, b1 in todo:
            m0, m1 = rows[b0], rows[b1]
            frames, arena = next(fresh)
            frame_of = [i - b0 for i in range(b0, b1) for _ in range(counts[i])]
            out = None
            if m1 > m0:
                crop_w = paste_w = wins[m0:m1]
                if tracked:
                    # the boxes of the batch's rows (row i: frame t of stream s), one upload and ONE launch for the batch
                    of_row, boxes = [s for s, _ in order[b0:b1]], []
                    for s, t in order[b0:b1]:
                        box = next(box_readers[s], None)
                        if box is None:
                            raise ValueError(f"stream {s}: its 'boxes' ended before its frames did, at frame {t}")
                        boxes.append(box.to(self.device).double())
                    sizes = [frames_mod.frame_size(f[None], plan.fmt[0])[::-1] for f in frames]
                    crop_w, paste_w = self._track(crop_states, torch.stack(boxes), torch.tensor(of_row, dtype=torch.int32).to(self.device),
                                                  sizes, plan, m0)
                crops = ops.crop_faces_mixed(frames, S, crop_w, frame_of, *plan.fmt)
                ident = None if ids_dev is None else ids_dev[m0:m1]
                out, m = self._drive_crops(crops, frames_mod.RowsAt(ident, m0, m1 - m0, ident, None), plan, smooth=smooth_pose)
                if paste_back:
                    ops.paste_faces_mixed(frames, out, paste_w, frame_of, feather, m, *plan.fmt)
            if paste_back:
                meta, out = [(s, t, tuple(f.shape)) for (s, t), f in zip(order[b0:b1], frames)], arena
            else:
                meta = [(s, t, counts[i]) for i, (s, t) in zip(range(b0, b1), order[b0:b1])]
            if host_ring is not None:
                for tag, buf in host_ring.push(meta, out):
                    yield handed_out(tag, buf)
            else:
                yield handed_out(meta, out)
        if host_ring is not None:
            for tag, buf in host_ring.drain():
                yield handed_out(tag, buf)

    def share_source(self, src_rank=0):
        """RCCL broadcast of the per-identity cache computed on `src_rank`: canonical volume
        (25 MB) + idt_embed (32 KB) + source theta."""
        c, d, s = self.cfg["latent_volume_channels"], self.cfg["latent_volume_depth"], self.cfg["latent_volume_size"]
        # idt_embed is [1, idt_output_channels, idt_output_size, idt_output_size] of the checkpoint's embedder config: the
        # receivers learn its shape from the broadcast header; what the warp embedding needs is checked on the source rank
        es = self.cfg["gen_embed_size"]
        # the source expression (the expression controls' neutral) travels with it; an identity without one sends an empty row
        expr = self.pred_source_pose_embed
        expr = torch.zeros((1, 0), device=self.device) if expr is None else expr.reshape(1, -1)
        # ... and so does the source (scale, rotation, translation), the head-pose controls' source pose
        srt = torch.zeros((1, 0), device=self.device) if self.pred_source_srt is None else self.pred_source_srt.reshape(1, 9)
        cache = parallel.broadcast_source_cache(
            dict(canonical=self.target_latent_volume, idt_embed=self.idt_embed, theta_src=self.pred_source_theta, expr_src=expr,
                 srt_src=srt),
            shapes=dict(canonical=(1, c, d, s, s), theta_src=(1, 4, 4)),
            names=['canonical', 'idt_embed', 'theta_src', 'expr_src', 'srt_src'],
            src=src_rank, device=self.device, world=self.world, rank=self.rank)
        if cache["idt_embed"].numel() != self.cfg["gen_max_channels"] * es * es:
            raise RuntimeError(f"idt_embed {tuple(cache['idt_embed'].shape)} does not match the warp embedding "
                               f"({self.cfg['gen_max_channels']} channels x {es}x{es})")
        self.pred_source_theta = cache["theta_src"]
        self.pred_source_pose_embed = cache["expr_src"].clone() if cache["expr_src"].numel() else None
        self.pred_source_srt = cache["srt_src"].clone() if cache["srt_src"].numel() else None
        self._stream.restart(pose_anchor=True)
        self._set_source_cache(canonical=cache["canonical"], idt_embed=cache["idt_embed"])
