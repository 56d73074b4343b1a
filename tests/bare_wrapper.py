"""TEST INFRASTRUCTURE ONLY -- the bare InferenceWrapper of the emulated tests, built in one place: an object without models on CPU
tensors, in front of a host-compiled library (tests/counting_lib.CountingLib over tests/emul/emulibs), whose driver pass records what
it is handed.  `patch` is anything with pytest's monkeypatch.setattr(target, name, value)."""
import torch

CFG = dict(latent_volume_channels=4, latent_volume_depth=2, latent_volume_size=2, gen_embed_size=1, gen_max_channels=4, image_size=8)


def bare_wrapper(patch, lib, capacity, **cfg):
    """an InferenceWrapper with a `capacity`-slot bank of the smallest shapes and everything but the driver pass, which appends
    (pose, theta, identity or None) to w.recorded and returns a black image; hip.load() hands out `lib`"""
    from emoportraits_amd import hip
    from emoportraits_amd.infer import InferenceWrapper
    patch.setattr(hip, "load", lambda: lib)
    patch.setattr(hip, "require_cuda_f32", lambda *a, **k: None)
    patch.setattr(hip, "current_stream", lambda: None)
    w = object.__new__(InferenceWrapper)
    w.device, w.rank, w.world = torch.device("cpu"), 0, 1
    w.cfg = dict(CFG, **cfg)
    w._init_state(use_graphs=False, identity_capacity=capacity, pose_momentum=0.3)
    w.embedders = {}
    w.lib = lib
    w.recorded = []

    def drive(pose, theta, ident=None):
        w.recorded.append((pose.clone(), theta.clone(), None if ident is None else ident.clone()))
        return torch.zeros(pose.shape[0], 3, w.cfg["image_size"], w.cfg["image_size"])
    w._drive_bank = drive
    w._drive = lambda pose, theta: drive(pose, theta)
    return w


def host_uploads(patch, seen=None):
    """frames.uploaded / uploaded_mixed as plain host copies (the mixed one into an arena, as the product lays it out), the copy
    stream none, the byte -> fp32 unpacking (an op that insists on device memory) torch's; seen(n): called with the number of frames
    of every upload as it is made"""
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import ops
    seen = seen or (lambda n: None)

    def uploaded(chunk, spans, device, stream):
        for a, b in spans:
            seen(b - a)
            yield a, b, chunk[a:b].clone().as_subclass(torch.Tensor)     # (a plain tensor, whatever stand-in the chunk is)

    def uploaded_mixed(batches, device, stream, copy_all):
        for batch in batches:
            shapes = [tuple(f.shape) for f in batch]
            offsets, total = frames_mod.arena_layout(shapes)
            arena = torch.zeros(total, dtype=torch.uint8)
            views = frames_mod.arena_views(arena, shapes, offsets)
            for v, f in zip(views, batch):
                v.copy_(f)
            seen(len(batch))
            yield views, arena
    patch.setattr(torch.cuda, "Stream", lambda device=None: None)
    patch.setattr(ops, "unpack_rgb8", lambda u8: (u8.permute(0, 3, 1, 2).float() / 255).contiguous())
    patch.setattr(frames_mod, "uploaded", uploaded)
    patch.setattr(frames_mod, "uploaded_mixed", uploaded_mixed)
