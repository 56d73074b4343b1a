"""Host-side executors of the hot-path networks on top of the HIP kernels (emoportraits_amd/ops.py).

Each class mirrors one reference module (same constructor inputs: a RAW reference state_dict + key prefix, so
released checkpoints drop in), folds spectral norm / weight standardisation once, packs the conv weights for the
implicit-GEMM kernel, and replays the module's forward as a sequence of kernel launches:

    reference module (file:line)                                               here
    ResBlock                networks/volumetric_avatar/utils.py:661-788         ResBlock
    WarpGenerator           networks/volumetric_avatar/warp_generator_resnet.py WarpGenerator
    Decoder + ImageDecoder  networks/volumetric_avatar/decoder.py:20-410        Decoder
    LocalEncoder            networks/volumetric_avatar/local_encoder.py:26-125  LocalEncoder
    VPN_ResBlocks           vpn_resblocks.py:22-49, resblocks_3d.py:9-62        VPNResBlocks
    Unet3D                  networks/volumetric_avatar/unet_3d.py:18-290        Unet3D
    Model.predict_embed     models/stage_1/volumetric_avatar/va.py:813-885      WarpEmbed

There is no torch compute here: torch only owns the buffers.  Every op raises if the HIP library is missing.
"""
import math
import os

import torch

from . import ops
from .pack import PackedConv, fold_sn


def _dev(t, device):
    return t.detach().float().contiguous().to(device)


class Norm:
    """nn.GroupNorm(32, C) (statistics reduced on the GPU per call) or eval-mode nn.BatchNorm (a static per-channel
    affine folded at load time: stage 2 with its default flags) -> (scale, shift) [N,C] for the conv staging."""

    def __init__(self, sd, prefix, device):
        self.gamma, self.beta = _dev(sd[prefix + ".weight"], device), _dev(sd[prefix + ".bias"], device)
        self.bn = (prefix + ".running_mean") in sd
        if self.bn:
            rm, rv = sd[prefix + ".running_mean"].double(), sd[prefix + ".running_var"].double()
            sc = sd[prefix + ".weight"].double() / torch.sqrt(rv + 1e-5)      # nn.BatchNorm2d eps
            sh = sd[prefix + ".bias"].double() - rm * sc
            self.scale, self.shift = _dev(sc.float()[None], device), _dev(sh.float()[None], device)

    def affine(self, x, ada=None, stats=None):
        """stats: ops.TileStats of x left behind by the conv that produced it (then x is not read again)"""
        if self.bn:
            n = x.shape[0]
            return self.scale.expand(n, -1).contiguous(), self.shift.expand(n, -1).contiguous()
        a = ada or (None, None)
        return ops.groupnorm_affine(x, self.gamma, self.beta, a[0], a[1], stats=stats)


class ResBlock:
    """GN -> ReLU -> conv3 -> GN -> ReLU -> conv3 (+ skip), utils.py:661-788.

    first_kind: 'ws' where the reference's WS replacement hit block_feats.2 (utils.py:1061-1096), else 'sn'.
    The GroupNorm-apply + ReLU in front of each conv is folded into the conv's input staging; nearest x2
    upsampling (decoder up-blocks) is folded into the conv's gather; the skip sum is the conv epilogue."""

    def __init__(self, sd, prefix, first_kind, device):
        self.prefix = prefix
        self.conv1 = PackedConv.from_state_dict(sd, prefix + ".block_feats.2", first_kind, device)
        self.conv2 = PackedConv.from_state_dict(sd, prefix + ".block.0", "sn", device)
        self.skip = None
        if (prefix + ".skip.0.weight_orig") in sd:
            self.skip = PackedConv.from_state_dict(sd, prefix + ".skip.0", "sn", device)
        self.n1 = Norm(sd, prefix + ".block_feats.0", device)
        self.n2 = Norm(sd, prefix + ".block_feats.3", device)

    def __call__(self, x, ups=False, ada1=None, ada2=None, down=None, x_stats=None, want_stats=False):
        """x: block input (pre-upsample when ups).  ada1/ada2: (ada_gamma, ada_beta) [N,C] views or None.
        down: avg-pool kernel applied to the block output.  The reference pools the main and the skip branch
        separately before adding them (utils.py:744-760); pooling is linear, so pool(main + skip) is the same
        function evaluated with one pooling pass instead of two.
        x_stats: ops.TileStats of x (from the conv that produced it); want_stats: return (out, TileStats of out) -- the
        GroupNorm statistics travel with the tensors instead of being reduced by a separate pass over them."""
        # GroupNorm statistics are invariant under nearest x2 upsampling (every element is replicated 4x),
        # so they are those of the small pre-upsample tensor
        need = not self.n1.bn
        s1, h1 = self.n1.affine(x, ada1, stats=x_stats)
        h, hst = ops.conv_igemm(x, self.conv1, s1, h1, relu_in=True, ups=ups, want_stats=True) if need else \
            (ops.conv_igemm(x, self.conv1, s1, h1, relu_in=True, ups=ups), None)
        s2, h2 = self.n2.affine(h, ada2, stats=hst)
        ws = want_stats and down is None and need
        if self.skip is not None and ups and (self.skip.kh, self.skip.kw, self.skip.kd) == (1, 1, 1):
            # a 1x1 convolution commutes with nearest upsampling: conv1x1(up(x)) == up(conv1x1(x)) element for element
            # (same dot product, same order), so the skip runs on the small tensor -- a quarter of the work -- and the
            # epilogue of conv2 reads it at (y>>1, x>>1)
            r = ops.conv_igemm(x, self.skip)
            out = ops.conv_igemm(h, self.conv2, s2, h2, relu_in=True, res=r, res_ups=True, want_stats=ws)
        elif self.skip is not None:
            r = ops.conv_igemm(x, self.skip, ups=ups)
            # (no out=r: the guarded recomputation of a range-checked layer reads the residual a second time)
            out = ops.conv_igemm(h, self.conv2, s2, h2, relu_in=True, res=r, want_stats=ws)
        else:
            out = ops.conv_igemm(h, self.conv2, s2, h2, relu_in=True, res=x, res_ups=ups, want_stats=ws)
        ost = None
        if ws:
            out, ost = out
        if down is not None:
            out = ops.avgpool(out, down)
        return (out, ost) if want_stats else out


class WarpEmbed:
    """Model.predict_embed, warp-embedding branch (va.py:813-885): Linear(pose) -> (+idt)*0.5 -> 1x1 conv."""

    def __init__(self, sd, cfg, device):
        self.es = cfg["gen_embed_size"]
        self.w_lin = _dev(sd["pose_unsqueeze_nw.weight"], device)                       # [C*es*es, E]
        w = fold_sn(sd["warp_embed_head_orig_nw.weight_orig"].float(), sd["warp_embed_head_orig_nw.weight_u"].float(),
                    sd["warp_embed_head_orig_nw.weight_v"].float())
        self.w_head = _dev(w.reshape(w.shape[0], w.shape[1]), device)                   # [C, C]

    def __call__(self, pose_embed, idt_embed, identity=None):
        """pose_embed [B,E], idt_embed [1,C,es,es] -> warp embed [B, C, es*es].  With identity (int32 [B] on the device),
        idt_embed is a bank [K,C,es,es] and row b adds idt_embed[identity[b]]"""
        B = pose_embed.shape[0]
        nn = self.es * self.es
        e = ops.small_gemm(self.w_lin, pose_embed.reshape(B, -1, 1), 1)                  # [B, C*nn, 1]
        if identity is not None:
            x = ops.add_rows_indexed(e, idt_embed.reshape(idt_embed.shape[0], -1, 1), identity, 0.5)
        else:
            x = ops.add(e, idt_embed.reshape(-1), 0.5)                                   # (e + idt) * 0.5
        return ops.small_gemm(self.w_head, x.view(B, -1, nn), nn)                        # [B, C, nn]


class WarpGenerator:
    """warp_generator_resnet.py:38-181.  __call__ returns the planar deltas [B,3,d,s,s]; the sampler adds the
    identity lattice itself (grid_kind=1), so `warp` is never materialised."""

    def __init__(self, sd, prefix, cfg, device):
        self.prefix = prefix
        nb = int(math.log(cfg["warp_output_size"] // cfg["gen_embed_size"], 2))
        f = lambda i: min(int(cfg["gen_num_channels"] * cfg["warp_channel_mult"] * 2 ** i), cfg["gen_max_channels"]) // 32 * 32
        self.chans = [f(nb)] + [f(i) for i in range(nb - 1, -1, -1)]
        self.inp = cfg["gen_embed_size"]
        self.out_depth = cfg["gen_latent_texture_depth"]
        self.n_depth_resize = int(math.log(cfg["gen_latent_texture_size"] // self.inp, 2))
        w = fold_sn(sd[prefix + ".first_conv.weight_orig"].float(), sd[prefix + ".first_conv.weight_u"].float(),
                    sd[prefix + ".first_conv.weight_v"].float())
        self.w_first = _dev(w.reshape(w.shape[0], w.shape[1]), device)
        self.blocks = [ResBlock(sd, f"{prefix}.blocks_3d.{i}", "ws", device) for i in range(nb)]
        # ProjectorNorm (utils.py:1113-1151): rows of all adaptive norms concatenated
        us, vs, rows, gam, bet = [], [], [], [], []
        self.slices = []
        off = 0
        for i in range(2 * nb):
            u = sd[f"{prefix}.projector.u.{i}"].float()
            us.append(u)
            vs.append(sd[f"{prefix}.projector.v.{i}"].float())
            rows += [i] * u.shape[0]
            blk, which = divmod(i, 2)
            npre = f"{prefix}.blocks_3d.{blk}.block_feats.{0 if which == 0 else 3}"
            gam.append(sd[npre + ".weight"].float())
            bet.append(sd[npre + ".bias"].float())
            self.slices.append((off, off + u.shape[0]))
            off += u.shape[0]
        self.u_all = _dev(torch.cat(us), device)                                         # [R, 512]
        self.v_all = _dev(torch.stack(vs), device)                                       # [2nb, E, 2]
        self.norm_of_row = torch.tensor(rows, dtype=torch.int32, device=device)
        self.gamma_all, self.beta_all = _dev(torch.cat(gam), device), _dev(torch.cat(bet), device)
        self.nh = Norm(sd, prefix + ".pre_head.0", device)
        self.head = PackedConv.from_state_dict(sd, prefix + ".head.0.0", "sn", device)

    def __call__(self, embed):
        """embed [B, C, es*es] -> deltas [B, 3, d, s, s]"""
        B = embed.shape[0]
        nn = embed.shape[2]
        T = ops.small_gemm(self.u_all, embed, nn)                                        # [B, R, nn]
        ag, ab = ops.projector_finalize(T, self.v_all, self.norm_of_row, self.gamma_all, self.beta_all)
        x = ops.small_gemm(self.w_first, embed, nn)                                      # [B, C0*inp, nn]
        inp = self.inp
        x = x.view(B, -1, inp, inp, inp)
        size = [inp, inp, inp]
        for i, blk in enumerate(self.blocks, 1):
            size[1] *= 2
            size[2] *= 2
            depth_new = min(self.out_depth * 2 ** (self.n_depth_resize - i), size[1]) if i < self.n_depth_resize else self.out_depth
            up, down = depth_new > size[0], depth_new < size[0]
            size[0] = depth_new
            # (the block's first norm takes its statistics from the upsampling kernel: no pass of its own over the big tensor)
            fac = (2, 2, 2) if up else (1, 2, 2)
            x, xs = (ops.upsample_trilinear(x, fac), None) if blk.n1.bn else ops.upsample_trilinear(x, fac, gn_groups=32)
            (a0, a1), (b0, b1) = self.slices[2 * (i - 1)], self.slices[2 * (i - 1) + 1]
            x = blk(x, ada1=(ag[:, a0:a1], ab[:, a0:a1]), ada2=(ag[:, b0:b1], ab[:, b0:b1]), x_stats=xs)
            if down:
                x = ops.avgpool(x, (2, 1, 1))
        s, h = self.nh.affine(x)
        return ops.conv_igemm(x, self.head, s, h, relu_in=True, act="tanh")


class Decoder:
    """decoder.py: res_decoder (1x1 + dec_num_blocks ResBlocks @ latent size) + ImageDecoder up-stages + sigmoid head."""

    def __init__(self, sd, prefix, cfg, device):
        nup = int(math.log(cfg["image_size"] // cfg["gen_latent_texture_size"], 2))
        self.first = PackedConv.from_state_dict(sd, prefix + ".res_decoder.0", "sn", device)
        self.trunk = [ResBlock(sd, f"{prefix}.res_decoder.{i + 1}", "ws", device) for i in range(cfg["dec_num_blocks"])]
        self.up = []
        k = 0
        for _ in range(nup):
            for j in range(cfg["im_dec_num_lrs_per_resolution"]):
                self.up.append((ResBlock(sd, f"{prefix}.img_decoder.dec_img_blocks.{k}", "ws", device), j == 0))
                k += 1
        hp = prefix + ".img_decoder.dec_img_head"
        self.nh = Norm(sd, hp + ".0", device)
        self.head = PackedConv.from_state_dict(sd, hp + ".2", "ws", device)

    def __call__(self, feat_2d):
        """feat_2d [B, c*d, s, s] -> (img [B,3,S,S], feat_2d after res_decoder, img_feat) as stage_two=True returns"""
        x, st = ops.conv_igemm(feat_2d, self.first, want_stats=True)
        for blk in self.trunk:
            x, st = blk(x, x_stats=st, want_stats=True)
        feat = x
        for blk, ups in self.up:
            x, st = blk(x, ups=ups, x_stats=st, want_stats=True)
        s, h = self.nh.affine(x, stats=st)
        img = ops.conv_head(x, self.head, s, h, relu_in=True, act="sigmoid")       # 3 output channels: a stream, not a GEMM
        return img, feat, x


class VPNResBlocks:
    """vpn_resblocks.py / resblocks_3d.py: plain GroupNorm => both convs keep spectral norm."""

    def __init__(self, sd, prefix, cfg, device):
        self.blocks = [ResBlock(sd, f"{prefix}.net.net.{i}", "sn", device) for i in range(cfg["source_volume_num_blocks"])]

    def __call__(self, vol, stats=None):
        for b in self.blocks:
            vol, stats = b(vol, x_stats=stats, want_stats=True)
        return vol


class Unet3D:
    """unet_3d.py:44-290 (released flags: no adaptive layers, learned constant input, skip ResBlocks)."""

    def __init__(self, sd, prefix, cfg, device):
        self.nb = int(math.log(cfg["gen_latent_texture_size"] // cfg["gen_dummy_input_size"], 2))
        self.depth = cfg["gen_latent_texture_depth"]
        self.down = [ResBlock(sd, f"{prefix}.blocks_3d_down.{i}", "sn", device) for i in range(self.nb)]
        self.up = [ResBlock(sd, f"{prefix}.blocks_3d_up.{i}", "sn", device) for i in range(self.nb)]
        self.skipb = [ResBlock(sd, f"{prefix}.skip_blocks_3d_up.{i}", "sn", device) for i in range(self.nb)]
        self.input_tensor = _dev(sd[prefix + ".input_tensor"], device)
        self.nh = Norm(sd, prefix + ".head.0", device)
        self.head = PackedConv.from_state_dict(sd, prefix + ".head.2", "sn", device)

    def __call__(self, vol):
        nb = self.nb
        x = vol
        feats = []
        size = [self.depth, vol.shape[-1], vol.shape[-1]]
        for i in range(nb):
            up = down = False
            if i < nb - 1:
                size[1] //= 2
                size[2] //= 2
                depth_new = min(size[0] * 2, size[1])
                up, down = depth_new > size[0], depth_new < size[0]
                size[0] = depth_new
                if up:
                    x = ops.upsample_trilinear(x, (2, 1, 1))
            x, st = self.down[i](x, want_stats=True)
            feats.append((x, st))
            if i < nb - 1:
                x = ops.avgpool(x, (2, 2, 2) if down else (1, 2, 2))
        feats = feats[::-1]
        B = vol.shape[0]
        x = self.input_tensor.expand(B, -1, -1, -1, -1).contiguous()
        size = [x.shape[2], x.shape[3], x.shape[4]]
        for i, (feat, fst) in enumerate(feats, 1):
            size[1] *= 2
            size[2] *= 2
            depth_new = min(self.depth * 2 ** (nb - i), size[1])
            up, down = depth_new > size[0], depth_new < size[0]
            size[0] = depth_new
            x = ops.upsample_trilinear(x, (2, 2, 2) if up else (1, 2, 2))
            skip = self.skipb[i - 1](feat, x_stats=fst)
            x = self.up[i - 1](ops.add(x, skip))
            if down:
                x = ops.avgpool(x, (2, 1, 1))
        s, h = self.nh.affine(x)
        return ops.conv_igemm(x, self.head, s, h, relu_in=True)


# fp32 results in every mode below.  'f16x2' (default since round 4) runs the covered 3x3 layers on the fp16 matrix pipes -- the
# scaled operands as two fp16 terms, three products, fp32 accumulation: error against an fp64 convolution that of a plain fp32
# convolution -- with the operand range checked ON THE DEVICE by every launch and a guarded bf16x3 launch behind it that
# recomputes a layer whose check fired (ops.conv_igemm; include/emo_hip.h), so that no result ever depends on the range
# assumption.  'bf16x3' (round 3's default) runs the same layers as an exact three-way bf16 split, six products: no range to
# check, 1.45x the matrix work.  'f32' is the exact-fp32 MFMA kernel everywhere.  EMO_CONV_PRECISION selects.
DEFAULT_PRECISION = "f16x2"


class HotPath:
    """All hot-path networks of one checkpoint, resident on one GPU.

    driver_pass replays notebooks/infer.py:583-637 for a BATCH of driver frames sharing one source identity
    (the reference loops batch-1 calls, F5).  source_pass replays infer.py:433-507."""

    def __init__(self, state_dict, cfg, device="cuda:0", with_source=True, precision=None):
        """precision (None: EMO_CONV_PRECISION, else DEFAULT_PRECISION):
        'f32'    exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) in every convolution;
        'bf16x3' fp32 results on the bf16 matrix pipes in the 3x3 layers csrc/conv_igemm_bf16x3.h covers -- every operand split
                 exactly into three bf16 terms, six partial products, fp32 accumulation: held to the same parity bounds as 'f32'
                 (tests/test_conv_bf16x3_gpu.py, tests/test_bench_config_parity_gpu.py) -- exact-fp32 MFMA elsewhere;
        'f16x2'  the same layers with half the matrix work: the scaled operands as two fp16 terms, three products (error against
                 fp64 that of an fp32 convolution).  Its operand range (+-2047 after norm + ReLU) is checked on the device by
                 every launch; a guarded bf16x3 launch recomputes a layer whose check fired, so results never depend on it;
        'f16'    opt-in reduced precision (BASELINE configs[4]): fp16 MFMA operands with fp32 accumulation in the 3x3 / 1x1
                 convolutions; tensors in HBM stay fp32"""
        self.cfg = cfg
        self.device = torch.device(device)
        if precision is None:
            precision = os.environ.get("EMO_CONV_PRECISION", DEFAULT_PRECISION)
        self.precision = precision
        sd = state_dict
        self.pad = cfg["grid_sample_padding_mode"]
        self.c, self.d, self.s = cfg["latent_volume_channels"], cfg["latent_volume_depth"], cfg["latent_volume_size"]
        self.with_source = with_source
        # frames per sampler launch pair: the warped intermediate of a chunk (25 MB per frame) is consumed by the second
        # call while it is still in the 256 MiB Infinity Cache (measured: 27.1 -> 23.5 us per frame for the pair at 16 frames)
        self.sampler_chunk = int(os.environ.get("EMO_SAMPLER_CHUNK", "4"))
        self.sampler_uv_variant = int(os.environ.get("EMO_SAMPLER_UV_VARIANT", "0"))   # 1: 4x4x4 output bricks instead of rows (A/B)
        # 2: the aligned volume goes past the caches (non-temporal stores).  Measured inconclusive: - 5 % on the pair when every
        # launch is bracketed by events (archive/profiles/r3_sampler_nt_out_ab.jsonl), nothing back to back or in the bench
        # (archive/profiles/r3_sampler_microbench.jsonl): off
        self.sampler_rot_variant = int(os.environ.get("EMO_SAMPLER_ROT_VARIANT", "0"))
        from .pack import conv_precision
        # fp16 mode: the WarpGenerators keep fp32-accurate arithmetic (EMO_WARP_PRECISION=f16 overrides) -- their output is
        # GEOMETRY (where the volume is sampled): measured at R256, fp16 operands there put 2e-3 on the deltas and 2e-2 of max
        # on the warped volume, 10x the 1-2e-3 the decoder's own fp16 rounding causes (tools/diag_f16.py), for 10 % of the
        # time.  fp32-accurate means the range-checked fp16 SPLIT (round 6; 4.9 ms per 16 frames), not the fp32 MFMA kernel
        # (8.8 ms; EMO_WARP_PRECISION=f32 restores it): same deltas to 1e-5
        wprec = os.environ.get("EMO_WARP_PRECISION", "f16x2") if precision == "f16" else precision
        self.warp_precision = wprec
        with conv_precision(wprec):
            self.uv_generator = WarpGenerator(sd, "uv_generator_nw", cfg, self.device)
            if with_source:
                self.xy_generator = WarpGenerator(sd, "xy_generator_nw", cfg, self.device)
        with conv_precision(precision):
            self.embed = WarpEmbed(sd, cfg, self.device)
            self.decoder = Decoder(sd, "decoder_nw", cfg, self.device)
            if with_source:
                self.volume_source = VPNResBlocks(sd, "volume_source_nw", cfg, self.device)
                self.volume_process = Unet3D(sd, "volume_process_nw", cfg, self.device)
                from .encoder import LocalEncoder
                self.local_encoder = LocalEncoder(sd, "local_encoder_nw", cfg, self.device)

    def _clear_flags(self):
        """'f16x2': zero the overflow words of the fp16-split layers at the start of a pass (one fill kernel, stream-ordered,
        captured with the pass).  A word raised during the pass makes the guarded bf16x3 launch behind that layer recompute it
        (ops.conv_igemm); overflow_events() reports which layers did."""
        if "f16x2" in (self.precision, self.warp_precision):
            ops.clear_overflow_flags(self.device)

    def overflow_events(self):
        """{slot: layer name} of the fp16-split layers whose range check fired since the last pass started (host sync)"""
        return ops.overflow_events(self.device)

    # ---- per identity -------------------------------------------------------------------------------
    def source_pass(self, source_img_masked, idt_embed, source_pose_embed, theta_src, keep=False):
        """-> canonical volumes [B,c,d,s,s] (NCDHW, as the reference caches it in self.target_latent_volume) of B source
        identities: source_img_masked [B,3,S,S], idt_embed [B,C,es,es], source_pose_embed [B,E], theta_src [B,4,4].  Every
        launch takes the batch (per-sample idt rows, volumes and thetas); B = 1 is the reference's one identity per call."""
        c, d, s = self.c, self.d, self.s
        B = source_img_masked.shape[0]
        self._clear_flags()
        latents = self.local_encoder(source_img_masked)
        emb = self.embed(source_pose_embed, idt_embed)
        delta_xy = self.xy_generator(emb)
        # (the [B, c*d, s, s] -> [B, c, d, s, s] view regroups the channels: the 2-D tile statistics of `latents` do not
        # describe the 3-D GroupNorm groups, so the first VPN norm reduces its own)
        vol = self.volume_source(latents.view(B, c, d, s, s))
        inv = ops.mat4_inverse(theta_src.float().contiguous())            # infer.py:443 on the device: no host round trip
        # both sampler calls through the channels-last kernels (one repack in, NCDHW out): 2.5x the NCDHW gather's rate
        rot = ops.grid_sample3d(ops.volume_to_channels_last(vol), theta=inv, padding_mode=self.pad, in_layout="ndhwc",
                                out_layout="ndhwc")
        pre = ops.grid_sample3d(rot, delta=delta_xy, padding_mode=self.pad, in_layout="ndhwc", out_layout="ncdhw")
        canonical = self.volume_process(pre)
        if keep:
            return dict(latents=latents, warp_embed=emb, delta_xy=delta_xy, source_volume=vol, pre_canonical=pre,
                        canonical=canonical)
        return canonical

    def prepare_canonical(self, canonical):
        """channels-last copy of the cached canonical volume for the samplers (done once per identity)"""
        return ops.volume_to_channels_last(canonical)

    # ---- per driver batch ---------------------------------------------------------------------------
    def driver_pass(self, canonical_cl, idt_embed, target_pose_embed, theta_drv, keep=False, identity=None):
        """identity=None: one identity, canonical_cl [1,d,s,s,c] and idt_embed [1,C,es,es].  identity (int32 [B] on the device):
        frame b renders identity[b] of a bank, canonical_cl [K,d,s,s,c] and idt_embed [K,C,es,es] -- the warp embedding adds that
        row's idt_embed and the uv sampler reads that row's volume; every other launch is the same as without a bank."""
        B = target_pose_embed.shape[0]
        self._clear_flags()
        emb = self.embed(target_pose_embed, idt_embed, identity)
        delta_uv = self.uv_generator(emb)
        lay = "ndhwc"
        aligned = torch.empty((B, self.c, self.d, self.s, self.s), device=self.device, dtype=torch.float32)
        theta3 = theta_drv[:, :3].contiguous()
        step = self.sampler_chunk if self.sampler_chunk > 0 else B
        for a in range(0, B, step):
            b = min(B, a + step)
            warped = ops.grid_sample3d(canonical_cl, delta=delta_uv[a:b], padding_mode=self.pad, in_layout=lay, out_layout=lay,
                                       variant=self.sampler_uv_variant, vol_index=None if identity is None else identity[a:b])
            ops.grid_sample3d(warped, theta=theta3[a:b], padding_mode=self.pad, in_layout=lay, out_layout="ncdhw",
                              out=aligned[a:b], variant=self.sampler_rot_variant)
        feat = aligned.view(B, self.c * self.d, self.s, self.s)
        img, deep_f, img_f = self.decoder(feat)
        if keep:
            return dict(warp_embed=emb, delta_uv=delta_uv, aligned=aligned, img=img, deep_f=deep_f, img_f=img_f)
        return img
