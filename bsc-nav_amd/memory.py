"""VoxelTokenMemory — drop-in for the reference class of the same name (memory_2.py:38), backed by libbscnav.

Same constructor signature, method names, argument meaning and return types as the reference for the
memory construction / query path, so that BSCAgent.GESObjectNavRobot and create_memory_for_dataset.py can
hold this object instead.  What differs, by design:
  * the per-point Python loop, the HDF5 flush loop and the per-voxel scan run as HIP kernels;
  * simulator (NavEnv), detector (YOLO-World) and diffusion model are optional injected collaborators;
  * `feature_mode="exact"` keeps the reference's token-cache semantics bit for bit, `"mean"` / `"max"`
    are the dense per-voxel reductions (north-star mode) and are mergeable across GPUs.
"""
import os
import time

import numpy as np
import torch

from . import floors, store
from .config import from_namespace
from .engine import INT32_MIN, VoxelEngine
from .geometry import PoseChain, cam_mat_fov, sample_indices_fast as sample_indices

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class VoxelTokenMemory:
    def __init__(self, args, memory_path=None, init_state=None, build_map=False, preload_dino=None,
                 preload_yolo=None, need_diffusion=True, *, feature_mode="exact", env=None, imaginer=None,
                 token_dim=None, patch_size=None, voxel_capacity=None, token_capacity=None, gpu=0,
                 alpha_source=None, max_frames_per_call=1, quiet=True, fuse_encoder=False):
        self.args = args
        self.cfg = from_namespace(args)
        self.device = "cuda"                                    # memory_2.py:41
        if not torch.cuda.is_available():
            raise RuntimeError("VoxelTokenMemory (bsc_nav_amd) needs a ROCm GPU; there is no CPU path")
        self.gpu = gpu
        self.dinov2 = preload_dino                               # anything with forward_features(x)[...]
        self.yolow = preload_yolo
        self.imaginer = imaginer                                 # text -> list of images (memory_2.py:258-276)
        self.Env = env                                           # NavEnv-like collaborator (env.py:49)
        self.quiet = quiet
        self.feature_mode = feature_mode
        # exp(-r^2/1.2): "host" evaluates the reference's own NumPy expression (rgb bytes / weights bit-exact against the
        # reference), "device" uses the GPU's exp (last-ulp differences flip < 0.1 % of the truncated rgb bytes by one).
        # The reference-exact mode defaults to the exact setting; the dense north-star modes to the fast one.
        self.alpha_source = alpha_source or ("host" if feature_mode == "exact" else "device")
        self._gen = 0                                            # bumped by every call that changes the map
        self._export_cache = {}
        if memory_path:                                          # memory_2.py:61-64
            self.memory_save_path = memory_path
        else:
            self.memory_save_path = os.path.join(self.cfg.memory_path, self.cfg.scene_name)
        c = self.cfg
        self.patch_h = self.patch_w = int(patch_size or c.patch_size)          # memory_2.py:80-83
        self.n_patch_w = c.query_width // self.patch_w
        self.n_patch_h = c.query_height // self.patch_h
        if self.n_patch_w != self.n_patch_h:
            raise ValueError("square patch grids only (the reference reshapes to (n_patch_w, n_patch_h))")
        if fuse_encoder and preload_dino is not None and not hasattr(preload_dino, "patch_tokens"):
            # opt-in: the hub DINOv2 module's weights run through this library's own encoder (encoder.RandomViT: same architecture,
            # LayerScale folded).  fuse_encoder="f32": the reference's precision — f32 weights / activations / tokens, every dense
            # layer and attention on the fp16 matrix cores with split operands (tokens within 1e-5 of the PyTorch f32 module,
            # ~2.4x its speed); fuse_encoder=True / "bf16": bf16 weights and activations, library GEMMs — ~2.8x faster again,
            # NOT at the reference's precision
            from .encoder import RandomViT
            dt = torch.float32 if str(fuse_encoder).lower() in ("f32", "fp32", "float32") else torch.bfloat16
            self.dinov2 = RandomViT.from_dinov2_state_dict(preload_dino.state_dict(), image_size=c.query_height, dtype=dt).to(f"cuda:{gpu}")
        self.chain = PoseChain(c.base_forward_axis, c.base_left_axis, c.base_up_axis, c.base2cam_rot, c.sensor_height)
        self.base_transform = self.chain.base_transform
        self.base2cam_tf = self.chain.base2cam_tf
        self.cs = c.cell_size
        self.gs = int(c.grid_size)
        self.depth_sample_rate = c.depth_sample_rate
        self.calib_mat = cam_mat_fov(c.height, c.width, fov=90)                # memory_2.py:102
        self.min_depth, self.max_depth = c.min_depth, c.max_depth
        self.token_dim = int(token_dim or c.token_dim)
        self.iter_size, self.cache_size = c.iter_size, c.cache_size
        self.neighbor_radius = 1                                               # memory_2.py:113-115 (update_memory_surp_base)
        self.boring_threshold = 0.95
        self.surprise_threshold = 0.5
        # which update the full cache gets inside obs2voxeltoken (memory_2.py:880-881): "dist" (update_memory_dist_base, the
        # reference's line as shipped) or "surprise" (update_memory_surp_base with the three attributes above, read per call)
        self.flush_policy = getattr(args, "flush_policy", "dist")
        self.camera_height = c.sensor_height
        self.floor_height, self.map_height = c.floor_height, c.map_height
        self.maxh = int(self.map_height / self.cs)                             # memory_2.py:122-123
        self.minh = int(self.floor_height / self.cs)
        self.base_height = []
        self.long_memory_dict = []
        self.feat_path = None
        self._voxel_capacity = voxel_capacity
        self._token_capacity = token_capacity
        self._max_frames = max_frames_per_call
        self.engine = None
        self._make_engine()

    # ------------------------------------------------------------------------------------------
    def _make_engine(self):
        if self.engine is not None:
            self.engine.close()
        c = self.cfg
        self.engine = VoxelEngine(c.height, c.width, self.gs, self.cs, self.floor_height, self.map_height,
                                  self.n_patch_w, self.token_dim, mode=self.feature_mode, iter_size=self.iter_size,
                                  cache_size=self.cache_size, voxel_capacity=self._voxel_capacity,
                                  token_capacity=self._token_capacity, max_points=self._max_frames * c.height * c.width,
                                  device=self.gpu, min_depth=self.min_depth, max_depth=self.max_depth,
                                  min_h=self.minh, max_h=self.maxh)
        self._pushed_policy = ("dist",)                          # a new context flushes by distance
        self.chain.reset()
        self._touch()

    def _push_flush_policy(self):
        """The automatic flush of the coming ingest follows flush_policy / neighbor_radius / surprise_threshold /
        boring_threshold as they are now (exact mode; the engine is told only when the tuple changed)."""
        if self.feature_mode != "exact":
            return
        want = ("dist",) if self.flush_policy == "dist" else (
            self.flush_policy, int(self.neighbor_radius), float(self.surprise_threshold), float(self.boring_threshold))
        if want != getattr(self, "_pushed_policy", ("dist",)):
            self.engine.set_flush_policy(*want)
            self._pushed_policy = want

    def _log(self, *a):
        if not self.quiet:
            print(*a)

    # State the reference keeps as NumPy attributes (BSCAgent.py:179-218 reads them repeatedly).  Here it lives in HBM;
    # an export is one D2H copy (occupied_ids: 800 MB at the reference defaults), so exports are cached until the next
    # call that changes the map.
    def _touch(self):
        self._gen += 1
        self._export_cache.clear()

    def _cached(self, name, fn):
        """Cached exports are handed out READ-ONLY: the reference's attributes are its own mutable state, here they are
        snapshots of HBM, and an in-place edit by a caller would silently change every later read (copy to edit)."""
        hit = self._export_cache.get(name)
        if hit is None or hit[0] != self._gen:
            val = fn()
            for a in (val if isinstance(val, tuple) else (val,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            hit = (self._gen, val)
            self._export_cache[name] = hit
        return hit[1]

    @property
    def max_id(self):
        return self._cached("counters", self.engine.counters)["max_id"]

    @property
    def iter_id(self):
        return self._cached("counters", self.engine.counters)["iter_id"]

    @property
    def grid_rgb_pos(self):
        return self._cached("rgb", self.engine.export_rgb)[0]

    @property
    def grid_rgb(self):
        return self._cached("rgb", self.engine.export_rgb)[1]

    @property
    def weight(self):
        return self._cached("rgb", self.engine.export_rgb)[2]

    @property
    def occupied_ids(self):
        """(gs,gs,maxh-minh) i32 — a fresh D2H copy per read (800 MB at the reference defaults: not kept pinned in a cache)."""
        return self.engine.export_occupied()

    @property
    def cv_map(self):
        return self._cached("hmap", self.engine.export_heightmap)[1]

    @property
    def max_height(self):
        return self._cached("hmap", self.engine.export_heightmap)[0]

    @property
    def inv_init_base_tf(self):
        return [] if self.chain.inv_init_base_tf is None else self.chain.inv_init_base_tf

    # ------------------------------------------------------------------------------------------
    def initial_memory(self):
        """memory_2.py:298-309 — never overwrites: appends _1, _2, ... (split('_')[0] quirk kept)."""
        count = 1
        while os.path.exists(self.memory_save_path):
            self.memory_save_path = self.memory_save_path.split("_")[0]
            self.memory_save_path = f"{self.memory_save_path}_{count}"
            count += 1
        os.makedirs(self.memory_save_path)
        self.feat_path = self.memory_save_path + "/feat.h5df"
        self._log("memory init at:", self.memory_save_path)

    def get_total_token_count(self):
        """memory_2.py:312-323."""
        k = self.engine.counters()
        self._log("total_tokens:", k["store_tokens"])
        return k["store_tokens"]

    def update_memory_dist_base(self):
        """memory_2.py:326-358 — flush ALL iter_size cache rows into the per-voxel token store."""
        t1 = time.time()
        self.engine.flush()
        self._touch()
        self._log(f"finish updating, time:{time.time() - t1}")

    def update_memory_surp_base(self):
        """memory_2.py:364-536 — flush ALL iter_size cache rows by surprise against the neighbouring groups, then merge
        each changed group by similarity; reads neighbor_radius / surprise_threshold / boring_threshold at call time."""
        t1 = time.time()
        self.engine.flush_surprise(self.neighbor_radius, self.surprise_threshold, self.boring_threshold)
        self._touch()
        self._log(f"finish updating, time:{time.time() - t1}")

    # ------------------------------------------------------------------------------------------
    def _get_patch_token(self, img):
        """memory_2.py:732-742: u8 (H,W,3) -> /255 -> resize -> normalise -> patch tokens (g,g,D) on device."""
        x = torch.from_numpy(np.ascontiguousarray(img)).to(self.device).unsqueeze(0)
        x = x.permute(0, 3, 1, 2).float() / 255
        x = self._transform_tensor(x)
        with torch.no_grad():
            tok = self.dinov2.forward_features(x)["x_norm_patchtokens"].squeeze(0)
            tok = tok.reshape(self.n_patch_w, self.n_patch_h, -1)
        return tok

    def _batch_patch_tokens(self, rgb):
        """(F,H,W,C) u8 device frames -> (F,g,g,D) tokens: the encoder's fused batch entry when it has one
        (encoder.RandomViT.patch_tokens), otherwise the reference's forward_features contract (memory_2.py:732-742)."""
        if hasattr(self.dinov2, "patch_tokens"):
            return self.dinov2.patch_tokens(rgb)
        x = self._transform_tensor(rgb[..., :3].permute(0, 3, 1, 2).float() / 255)
        with torch.no_grad():
            tok = self.dinov2.forward_features(x)["x_norm_patchtokens"]
        return tok.reshape(rgb.shape[0], self.n_patch_w, self.n_patch_h, -1).float().contiguous()

    def _transform_tensor(self, x):
        """transform_ (memory_2.py:71-74): Resize((qh,qw)) on a float tensor (bilinear, antialias) + Normalize."""
        c = self.cfg
        if x.shape[-2:] != (c.query_height, c.query_width):
            x = torch.nn.functional.interpolate(x, size=(c.query_height, c.query_width), mode="bilinear",
                                                antialias=True, align_corners=False)
        mean = torch.tensor(IMAGENET_MEAN, device=x.device).view(1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD, device=x.device).view(1, 3, 1, 1)
        return (x - mean) / std

    def transform(self, pil_img):
        """transform (memory_2.py:66-70): PIL -> Resize -> ToTensor -> Normalize, (3,qh,qw) float."""
        from PIL import Image
        c = self.cfg
        img = pil_img.convert("RGB").resize((c.query_width, c.query_height), Image.BILINEAR)
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255
        mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1)
        std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
        return (x - mean) / std

    def _host_alpha(self, depth, idx):
        """exp(-r^2/1.2) evaluated exactly as the reference does on the host (memory_2.py:873-875, utils.py:153-173)."""
        h, w = depth.shape
        y, x = np.divmod(idx.astype(np.int64), w)
        p2d = np.vstack([x + 0.5, y + 0.5, np.ones_like(x, dtype=np.float64)])
        pc = (np.linalg.inv(self.calib_mat) @ p2d) * depth.reshape(-1)[idx].reshape(1, -1)
        r2 = (pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]
        return np.exp(-r2 / (2 * 0.6))

    def obs2voxeltoken(self, obs, pose):
        """memory_2.py:842-903 — one RGB-D frame into the memory."""
        T = self.chain.pc_transform(np.asarray(pose, dtype=np.float64))
        self.tf = self.chain.tf
        # the frame goes to the device ONCE and as it is (RGB or RGBA: the kernels read the first three channels, memory_2.py:853
        # `[:, :, :3]`) — stripping the alpha channel on the host was a strided 0.9 MB copy per frame, 0.4 ms of the 2.1
        rgb = np.asarray(obs["rgb"])
        if rgb.dtype != np.uint8 or not rgb.flags.c_contiguous or not rgb.flags.writeable:
            rgb = np.array(rgb, dtype=np.uint8, order="C")
        depth = np.ascontiguousarray(np.asarray(obs["depth"]), dtype=np.float32)
        d_rgb = torch.from_numpy(rgb).to(self.device).unsqueeze(0)
        patch_tokens = self._batch_patch_tokens(d_rgb).float().contiguous()
        idx = self._next_sample(depth.size)                                   # global NumPy RNG, as the reference
        alpha = None
        if self.alpha_source == "host":
            with np.errstate(all="ignore"):
                alpha = torch.from_numpy(self._host_alpha(depth, idx)).to(self.device)
        self._push_flush_policy()
        self.engine.ingest(torch.from_numpy(depth).to(self.device).unsqueeze(0), d_rgb, patch_tokens, T[None],
                           torch.from_numpy(idx).to(self.device), np.array([0, len(idx)], np.int64), alpha)
        self._touch()

    def _next_sample(self, n_pixels):
        pf = getattr(self, "_prefetcher", None)
        if pf is not None:
            if pf.n_pixels != n_pixels or pf.rate != self.depth_sample_rate:
                # drawing this frame from the global stream would be overwritten by close(): the two streams cannot be mixed
                raise ValueError(f"prefetched_sampling was opened for {pf.n_pixels} pixels at rate {pf.rate}; this frame has "
                                 f"{n_pixels} pixels at rate {self.depth_sample_rate} — close the prefetcher first")
            return pf.next()
        return sample_indices(n_pixels, self.depth_sample_rate)

    def prefetched_sampling(self, n_pixels=None, depth=4):
        """Context manager: while it is open, the shuffled sub-sampling of the coming frames is drawn ahead on a host thread
        (geometry.SamplePrefetcher) — same permutations, same final state of np.random's stream, the ~1 ms Fisher-Yates of
        frame f + 1 under the GPU work of frame f.  For loops that own np.random between frames (the dataset loop)."""
        import contextlib
        from .geometry import SamplePrefetcher

        @contextlib.contextmanager
        def ctx():
            self._prefetcher = SamplePrefetcher(n_pixels or self.cfg.height * self.cfg.width, self.depth_sample_rate, depth)
            try:
                yield self
            finally:
                pf, self._prefetcher = self._prefetcher, None
                pf.close()
        return ctx()

    def ingest_frames(self, rgb, depth, poses, tokens=None):
        """Batched ingest (new): rgb (F,H,W,C) u8, depth (F,H,W) f32 device tensors, poses (F,7).
        Every pixel is ingested when depth_sample_rate == 1, otherwise the reference's shuffled sub-sampling
        is drawn per frame.  Tokens default to self.dinov2.patch_tokens(rgb)."""
        F = rgb.shape[0]
        Ts = np.stack([self.chain.pc_transform(p) for p in np.asarray(poses, dtype=np.float64)])
        if tokens is None:
            tokens = self._batch_patch_tokens(rgb)
        self._touch()
        self._push_flush_policy()
        host_alpha = self.alpha_source == "host"
        if self.depth_sample_rate == 1 and self.feature_mode != "exact" and not host_alpha:
            self.engine.ingest(depth, rgb, tokens, Ts)
            return
        N = depth.shape[1] * depth.shape[2]
        idxs = [self._next_sample(N) for _ in range(F)]
        off = np.concatenate([[0], np.cumsum([len(i) for i in idxs])]).astype(np.int64)
        alpha = None
        if host_alpha:          # same setting as obs2voxeltoken: rgb bytes / weights bit-exact (one D2H copy of the depth)
            dh = depth.detach().cpu().numpy()
            with np.errstate(all="ignore"):
                alpha = torch.from_numpy(np.concatenate([self._host_alpha(dh[f], idxs[f]) for f in range(F)])).to(self.device)
        self.engine.ingest(depth, rgb, tokens, Ts, torch.from_numpy(np.concatenate(idxs)).to(self.device), off, alpha)

    # ------------------------------------------------------------------------------------------
    def imaginary(self, text_prompts, vis=False):
        """memory_2.py:258-276 — text -> images; the generator is an injected collaborator here."""
        if self.imaginer is None:
            raise RuntimeError("text prompts need an image generator: pass imaginer=callable(text, n) -> images "
                               "(the reference uses Stable-Diffusion-3.5, memory_2.py:258-276)")
        return self.imaginer(text_prompts, self.cfg.imagenary_num)

    def _query_embedding(self, prompt):
        """memory_2.py:566-608: prompt -> pooled (1,D) query on the device."""
        if isinstance(prompt, torch.Tensor) and prompt.dim() <= 2:
            return prompt.to(self.device, torch.float32).reshape(-1, self.token_dim)[:1].contiguous()
        if isinstance(prompt, torch.Tensor) and prompt.dim() == 3:                 # (B,T,D) patch tokens
            tokens = prompt.to(self.device, torch.float32).contiguous()
        else:
            if isinstance(prompt, str):
                imgs = self.imaginary(prompt)
                imgs = getattr(imgs, "images", imgs)
                x = torch.stack([i if isinstance(i, torch.Tensor) else self.transform(i) for i in imgs])
            elif isinstance(prompt, torch.Tensor):                                  # (B,3,H,W) already transformed
                x = prompt
            else:
                x = torch.stack([self.transform(prompt)])
            with torch.no_grad():
                tokens = self.dinov2.forward_features(x.to(self.device))["x_norm_patchtokens"].float().contiguous()
        return self.engine.pool_query(tokens).reshape(1, -1)

    def voxel_localized(self, prompt, K=100, batch_size=300, region_radius=np.inf, curr_grid=None):
        """memory_2.py:563-671 -> (top1 (1,3), positions (K,3) int64, similarities (K,) float64)."""
        t1 = time.time()
        q = self._query_embedding(prompt)
        radius = None if region_radius == np.inf else float(region_radius)
        floor = None
        if getattr(self.args, "load_single_floor", False) and hasattr(self, "floor_min_height"):
            floor = (self.floor_min_height, self.floor_max_height)
        pos, sim, cnt = self.engine.localize(q, K=K, radius=radius, curr=curr_grid, floor=floor)
        n = int(cnt[0])
        if n == 0:
            raise IndexError("list index out of range")          # the reference indexes top_k_positions[0]
        top_pos = pos[0, :n].astype(np.int64)
        top_sim = sim[0, :n].astype(np.float64)
        self._log(f"finish localizing, time:{time.time() - t1}")
        return np.array([top_pos[0]]), top_pos, top_sim

    def voxel_localized_batch(self, prompts, K=100, region_radius=np.inf, curr_grid=None, floors=None):
        """voxel_localized for several prompts in one call, each inside its own region (the adaptive-region loop of
        BSCAgent.py:1078-1098, the augmented prompts of working_memory_retrival, one position per agent of a shared map).
        prompts        list of whatever voxel_localized accepts, or a (Q,D) tensor of pooled embeddings;
        region_radius  one value for all or one per prompt (np.inf / None: no sphere);
        curr_grid      (3,) for all or (Q,3);
        floors         None: the loaded single floor for every query exactly when voxel_localized applies it
                       (args.load_single_floor); a list of (lo, hi) / None per prompt overrides it.
        -> list of (top1 (1,3), positions (n,3) int64, similarities (n,) float64), one per prompt.  Unlike voxel_localized,
        which raises IndexError like the reference, a prompt whose region holds no voxel gives empty arrays and a top1 of
        shape (0,3): one empty region must not lose the other answers."""
        t1 = time.time()
        if isinstance(prompts, torch.Tensor) and prompts.dim() == 2:
            q = prompts.to(self.device, torch.float32).contiguous()
        else:
            q = torch.cat([self._query_embedding(p) for p in prompts], 0)
        Q = q.shape[0]
        if floors is None and getattr(self.args, "load_single_floor", False) and hasattr(self, "floor_min_height"):
            floors = [(self.floor_min_height, self.floor_max_height)] * Q
        pos, sim, cnt = self.engine.localize_regions(q, K=K, radius=region_radius, curr=curr_grid, floor=floors)
        out = []
        for i in range(Q):
            n = int(cnt[i])
            top_pos = pos[i, :n].astype(np.int64)
            out.append((top_pos[:1], top_pos, sim[i, :n].astype(np.float64)))
        self._log(f"finish localizing {Q} prompts, time:{time.time() - t1}")
        return out

    def voxel_score_map(self, prompts, region_radius=np.inf, curr_grid=None, floors=None):
        """The field voxel_localized_batch ranks from: for every prompt the best score per top-down cell (r, c) and the height
        of the voxel that has it (VoxelEngine.score_map) — a value map for a planner, a heat map over cv_map.  prompts,
        region_radius, curr_grid and floors follow voxel_localized_batch, the loaded single floor (args.load_single_floor)
        included -> (score (Q,gs,gs) f32, height (Q,gs,gs) i32) torch tensors on the device; -inf / -1 where a prompt's
        region holds no voxel of the column."""
        if isinstance(prompts, torch.Tensor) and prompts.dim() == 2:
            q = prompts.to(self.device, torch.float32).contiguous()
        else:
            q = torch.cat([self._query_embedding(p) for p in prompts], 0)
        Q = q.shape[0]
        if floors is None and getattr(self.args, "load_single_floor", False) and hasattr(self, "floor_min_height"):
            floors = [(self.floor_min_height, self.floor_max_height)] * Q
        return self.engine.score_map(q, radius=region_radius, curr=curr_grid, floor=floors)

    def _default_band(self):
        """The loaded single floor's z-band exactly when voxel_localized applies it (args.load_single_floor), otherwise None."""
        if getattr(self.args, "load_single_floor", False) and hasattr(self, "floor_min_height"):
            return (self.floor_min_height, self.floor_max_height)
        return None

    def topdown_maps(self, bands=None):
        """Top-down maps of the stored voxels per height band (VoxelEngine.topdown_slices) — the floor plan voxel_score_map's
        field is laid over.  bands: a list of (lo, hi) stored heights / None (every height); None: the loaded single floor
        (args.load_single_floor) when one was selected, otherwise one open band
        -> dict(rgb (S,gs,gs,3) u8 in RGB order, height (S,gs,gs) i32, count (S,gs,gs) i32) torch tensors on the device."""
        if bands is None:
            bands = [self._default_band()]
        return self.engine.topdown_slices(bands)

    def _render(self, pose, size, fov, band, max_range, want):
        """render_view / visible_voxels: the engine call for one pose -> dict of CUDA tensors with the view axis dropped"""
        T = self.chain.transform_of(np.asarray(pose, dtype=np.float64))         # (the map does not move: chain.tf and the anchor stay)
        kinv = None
        if size is not None or fov is not None:
            h, w = (self.cfg.height, self.cfg.width) if size is None else (int(size[0]), int(size[1]))
            kinv = np.linalg.inv(cam_mat_fov(h, w, fov=90 if fov is None else fov))
        out = self.engine.render_views(T[None], size=size, kinv=kinv, band=self._default_band() if band is None else band,
                                       t_range=None if max_range is None else (self.min_depth, float(max_range)), want=want)
        return {k: (None if v is None else v[0]) for k, v in out.items()}

    def render_view(self, pose, size=None, fov=None, band=None, max_range=None):
        """The memory seen from `pose` (given as obs2voxeltoken takes it; VoxelEngine.render_views): per pixel the first stored
        voxel the ray meets -> dict(voxel (H,W) i32 ids, -1: none; depth (H,W) f32 in the parametrisation of a depth image, 0: none;
        rgb (H,W,3) u8 in RGB order) of NumPy arrays.  size (H, W) and fov build the intrinsics with cam_mat_fov (None, None: the
        frames' own; a quarter-size preview is size=(120, 160)); band (lo, hi) stored heights, None: the loaded single floor
        (args.load_single_floor) when one was selected, otherwise every height; max_range replaces max_depth.  The map does not
        move; RuntimeError before the first frame (there is no map frame to place the pose in)."""
        out = self._render(pose, size, fov, band, max_range, ("voxel", "depth", "rgb"))
        return {k: v.cpu().numpy() for k, v in out.items()}

    def visible_voxels(self, pose, size=None, fov=None, band=None, max_range=None):
        """The stored voxels in view at `pose` (arguments as render_view) -> (positions (n,3) int64 rows of grid_rgb_pos,
        pixel_counts (n,) int64: how many pixels show each), in ascending voxel id order."""
        ids = self._render(pose, size, fov, band, max_range, ("voxel",))["voxel"]
        ids, counts = torch.unique(ids[ids >= 0], return_counts=True)
        ids = ids.cpu().numpy().astype(np.int64)
        return np.asarray(self.grid_rgb_pos, np.int64)[ids].reshape(-1, 3), counts.cpu().numpy().astype(np.int64)

    def rgb_2d_map(self, height):
        """TrajectoryDrawer._get_rgb_2d_map (BSCAgent.py:203-234): per column the colour of the highest stored voxel at or below
        the cut floor(height / cs - minh) -> (gs,gs,3) uint8 NumPy array in BGR order, zeros where the column holds none."""
        cut = int(np.floor((height / self.cs) - self.minh))
        rgb = self.engine.topdown_slices([(INT32_MIN, cut)], heights=False, counts=False)["rgb"][0]
        return np.ascontiguousarray(rgb.cpu().numpy()[..., ::-1])

    def rebuild_topdown_map(self, band=None):
        """cv_map / max_height become the top-down map of the stored voxels inside `band` ((lo, hi); None: the default of
        topdown_maps) — what a memory from load_memory or merge_shards, whose map is empty, needs before the frontier calls
        (VoxelEngine.rebuild_topdown).  Nothing calls this on its own."""
        self.engine.rebuild_topdown(self._default_band() if band is None else band)
        self._touch()

    def weighted_cluster_centers(self, top_k_positions, top_k_similarity, eps=10, min_samples=5):
        """GESObjectNavRobot.weighted_cluster_centers (BSCAgent.py:479-497) on the GPU: DBSCAN over the top-K voxel
        positions + similarity-weighted centres -> (cluster_centers (n,3) f64, labels (K,), cluster_sizes)."""
        return self.engine.cluster_centers(top_k_positions, top_k_similarity, eps=eps, min_samples=min_samples)

    def weighted_cluster_centers_batch(self, positions, similarities, eps=10, min_samples=5):
        """weighted_cluster_centers for several top-K lists in one call: positions / similarities are lists of per-prompt
        arrays (n_i,3) / (n_i,) of any lengths (what voxel_localized_batch returns), or (Q,K,3) / (Q,K) arrays
        -> list of (cluster_centers (n,3) f64, labels (n_i,), cluster_sizes).  An empty list gives no clusters."""
        return self.engine.cluster_centers_batch(positions, similarities, eps=eps, min_samples=min_samples)

    def working_memory_retrieval_batch(self, prompts, K=100, region_radius=np.inf, curr_grid=None, floors=None, eps=10,
                                       min_samples=5, nearest_first=False):
        """The memory side of GESObjectNavRobot.working_memory_retrival (BSCAgent.py:587-664) for several prompts / regions
        in one go: voxel_localized_batch (same arguments, same rules) followed by weighted_cluster_centers on every
        prompt's top-K, which never leaves the GPU in between (two synchronizes for the whole batch).
        -> list of (cluster_centers (n,3) f64, top_k_positions (n_i,3) int64, top_k_similarity (n_i,) f64, labels (n_i,),
        cluster_sizes), one per prompt; a prompt whose region holds no voxel gives empty arrays.
        nearest_first  reorder each prompt's centres (and sizes) by their Euclidean distance to that prompt's curr_grid,
                       stable, as move2textprompt_adaptive_region does (BSCAgent.py:1086-1090); needs curr_grid.
        The adaptive-region loop (:1078-1098) is one call: prompts=[p, p, p], region_radius=(30, 40, 50), one curr_grid."""
        t1 = time.time()
        if nearest_first and curr_grid is None:
            raise ValueError("nearest_first orders the centres by distance to curr_grid")
        if isinstance(prompts, torch.Tensor) and prompts.dim() == 2:
            q = prompts.to(self.device, torch.float32).contiguous()
        else:
            q = torch.cat([self._query_embedding(p) for p in prompts], 0)
        Q = q.shape[0]
        if floors is None and getattr(self.args, "load_single_floor", False) and hasattr(self, "floor_min_height"):
            floors = [(self.floor_min_height, self.floor_max_height)] * Q
        pos, sim, cnt = self.engine.localize_regions(q, K=K, radius=region_radius, curr=curr_grid, floor=floors)
        clusters = self.engine.cluster_centers_batch(eps=eps, min_samples=min_samples)
        curr = None if curr_grid is None else np.broadcast_to(np.asarray(curr_grid, np.float64).reshape(-1, 3), (Q, 3))
        out = []
        for i in range(Q):
            n = int(cnt[i])
            centers, labels, sizes = clusters[i]
            if nearest_first and len(centers):
                order = np.argsort(np.linalg.norm(centers - curr[i], axis=1), kind="stable")
                centers, sizes = centers[order], [sizes[j] for j in order]
            out.append((centers, pos[i, :n].astype(np.int64), sim[i, :n].astype(np.float64), labels, sizes))
        self._log(f"finish retrieving {Q} prompts, time:{time.time() - t1}")
        return out

    def long_memory_filter(self):
        """memory_2.py:693-705."""
        if getattr(self.args, "load_single_floor", False) and hasattr(self, "floor_min_height"):
            return [o for o in self.long_memory_dict if self.floor_min_height <= o["loc"][2] <= self.floor_max_height]
        return self.long_memory_dict

    # ------------------------------------------------------------------------------------------
    def save_memory(self, original_pos=None):
        """The save block of exploring_create_memory (memory_2.py:1136-1145), plus the flat token store."""
        path = self.memory_save_path
        os.makedirs(path, exist_ok=True)
        pos, rgb, w = self.engine.export_rgb()
        if original_pos is None:
            original_pos = getattr(getattr(self.Env, "original_state", None), "position", np.zeros(3))
        store.save_rgb_state(path, pos, rgb, w, self.engine.export_occupied(), len(pos), original_pos, self.minh,
                             self.maxh, self.base_height, self.long_memory_dict)
        if self.feature_mode == "exact":
            store.save_token_store(path, *self.engine.export_store())
        else:
            store.save_dense(path, *self.engine.export_dense())

    # ---- frame-sharded builds (new: the reference is single-process) ---------------------------------
    def set_map_origin(self, pose):
        """Anchor the map frame at `pose` (the scene's first pose) on every rank of a frame-sharded build."""
        self.chain.anchor(pose)

    def enable_point_log(self, capacity_points):
        """Frame-sharded builds: keep 16 bytes per ingested point so that merge_shards reproduces rgb / weights bit for bit
        (dist.merge_colour_replay).  Meant for the sub-sampled modes (a few thousand points per frame); an every-pixel dense build
        may keep it too — 4.9 GB per 1 000 frames of 640x480, tested bit-exact at depth_sample_rate 1 — and pays a slower k_points
        and an all-to-all of its points at the merge.  Call on every rank before the first frame."""
        self.engine.point_log_enable(capacity_points)

    def merge_shards(self, group=None, root=0):
        """Dense modes: merge the per-rank maps (one reduce-scatter over RCCL, dist.merge_dense_maps) and collect the
        result on `root`, whose object then holds the whole memory — ids in the single-process first-touch order,
        features / counts reduced, rgb / weights exact when the ranks kept their points (enable_point_log), otherwise by the
        documented approximate rule, top-down map exact — ready for
        save_memory().  base_height and long_memory entries are concatenated in rank order.  -> True on root."""
        import torch.distributed as tdist
        from . import dist as bdist
        if self.feature_mode == "exact":
            raise RuntimeError("the exact (token-cache) mode is defined by the global point order: replicas only")
        info = bdist.merge_dense_maps(self.engine, group)
        self._touch()
        if not (tdist.is_available() and tdist.is_initialized()):
            return True
        is_root = bdist.gather_merged_to_root(self.engine, info, root, group)
        lists = [None] * tdist.get_world_size(group)
        tdist.all_gather_object(lists, (list(map(float, self.base_height)), self.long_memory_dict), group=group)
        if is_root:
            self.base_height = [h for bh, _ in lists for h in bh]
            self.long_memory_dict = [o for _, lm in lists for o in lm]
            self.long_memory_integration()
        self._touch()
        return is_root

    def load_memory(self, init_state=None, build_map=False):
        """memory_2.py:166-256."""
        if self.Env is not None and hasattr(self.Env, "reset"):
            self.Env.reset(self.args, init_state=init_state, build_map=build_map)
        self.memory_save_path = getattr(self.args, "load_memory_path", self.memory_save_path)
        self.base_height = []
        if build_map:
            self.engine.reset()
            self.chain.reset()
            self._touch()
            return
        path = self.memory_save_path
        st = store.load_rgb_state(path)
        tok = store.load_token_store(path) if self.feature_mode == "exact" else None
        remake = False
        if (st["minh"], st["maxh"]) != (self.minh, self.maxh):        # memory_2.py:200
            self.minh, self.maxh = st["minh"], st["maxh"]
            self.floor_height, self.map_height = self.minh * self.cs, self.maxh * self.cs
            remake = True
        # capacities follow the loaded memory (the reference store is bounded only by cache_size tokens per voxel):
        # room for the loaded voxels / tokens plus a few more cache flushes
        if len(st["pos"]) > self.engine.cfg.voxel_capacity:
            self._voxel_capacity = 2 * len(st["pos"])
            remake = True
        if tok is not None and len(tok[2]) + self.iter_size > self.engine.cfg.token_capacity:
            self._token_capacity = len(tok[2]) + 4 * self.iter_size
            remake = True
        if remake:
            self._make_engine()
        self.feat_path = path + "/feat.h5df"
        self.engine.import_rgb(st["pos"], st["rgb"], st["weight"])
        if tok is not None:
            self.engine.import_store(*tok)
        else:
            self.engine.import_dense(*store.load_dense(path))
        self._touch()
        self.long_memory_dict = st["long_memory"]
        self.original_pos = st["original_pos"]
        if self.Env is not None and hasattr(self.Env, "original_state"):
            self.Env.original_state.position = st["original_pos"]
        if getattr(self.args, "load_single_floor", False):
            self.base_height = st["base_height"]
            if self.Env is not None:
                current_height = self.Env.agent.get_state().position[1]
            else:
                current_height = float(st["original_pos"][1])
            self._select_floor(st["pos"], st["rgb"], current_height)

    def _select_floor(self, grid_rgb_pos, grid_rgb, current_height):
        """memory_2.py:202-252: floors from the recorded base heights, z-range of the floor the agent stands on, and the
        per-floor rgb voxel files the reference's viewers read (host logic in floors.py)."""
        sel = floors.select_floor(self.base_height, grid_rgb_pos, self.cs, current_height)
        self.floor_heights, self.num_floors = sel["levels"], sel["num_floors"]
        self.floor_min_height, self.floor_max_height = sel["zrange"]
        k = sel["current_floor"]
        np.save(self.memory_save_path + f"/grid_rgb_pos_floor_{k}.npy", grid_rgb_pos[sel["mask"]])
        np.save(self.memory_save_path + f"/grid_rgb_floor_{k}.npy", grid_rgb[sel["mask"]])
        return k

    # ------------------------------------------------------------------------------------------
    def long_memory(self, obs):
        """memory_2.py:905-945: detector boxes -> depth at the box centre -> voxel location -> {label, loc, confidence}.

        The detector (YOLO-World in the reference) is an injected collaborator: anything whose
        ``predict(PIL.Image, conf=...)`` returns ``[result]`` with ``result.boxes.{xyxy, conf, cls}``.  The geometry of the
        box-centre pixels runs through the same fp64 kernel as the voxel path (``bsc_geometry``)."""
        if self.yolow is None:
            return None
        from PIL import Image
        rgb = np.ascontiguousarray(np.array(obs["rgb"])[:, :, :3])
        self.yolow_results = self.yolow.predict(Image.fromarray(rgb), conf=getattr(self.args, "detect_conf", 0.55))
        boxes = self.yolow_results[0].boxes
        if len(boxes) > 0:
            depth = np.ascontiguousarray(np.array(obs["depth"]), dtype=np.float32)
            width = int(getattr(self.args, "width", depth.shape[1]))
            idx, confs, labels = [], [], []
            for i in range(len(boxes.conf)):
                xyxy = boxes.xyxy[i].cpu().numpy()
                col = int((xyxy[0] + xyxy[2]) / 2)
                row = int((xyxy[1] + xyxy[3]) / 2)
                idx.append(row * width + col)                                     # :917-919
                confs.append(boxes.conf[i].item())
                labels.append(self.args.detect_classes[int(boxes.cls[i].item())])
            T = self.chain.tf @ self.chain.base_transform @ self.chain.base2cam_tf   # :930 (pose of the last ingested frame)
            g = self.engine.geometry(torch.from_numpy(depth).to(self.device), T,
                                     torch.from_numpy(np.asarray(idx, dtype=np.int32)).to(self.device))
            for i in range(len(idx)):
                if not (g["flags"][i] & 1):        # :921 depth mask
                    continue
                if not (g["flags"][i] & 2):        # :935 _out_of_range
                    continue
                r, c, h = (int(v) for v in g["vox"][i])
                self.long_memory_dict.append({"label": labels[i], "loc": [r, c, h - self.minh], "confidence": confs[i]})
        self.long_memory_integration()

    def long_memory_integration(self, threshold=3):
        """memory_2.py:993-1025: per label, entries within L1 distance `threshold` merge, keeping the most confident."""
        groups = {}
        for item in self.long_memory_dict:
            groups.setdefault(item["label"], []).append(item)
        final = []
        for label, items in groups.items():
            kept = []
            for itm in items:
                for f in kept:
                    if sum(abs(a - b) for a, b in zip(f["loc"], itm["loc"])) <= threshold:
                        if itm["confidence"] > f["confidence"]:
                            f["loc"] = itm["loc"]
                            f["confidence"] = itm["confidence"]
                        break
                else:
                    kept.append(itm)
            final.extend(kept)
        self.long_memory_dict = final

    # ---- simulator-driven builds (memory_2.py:1086-1145): thin consumers of dataset.EnvExplorer's event stream ------------
    def _consume(self, events):
        """frames into the memory (+ the detector's long-term memory), goal heights into base_height"""
        for ev in events:
            if ev[0] == "frame":
                self.obs2voxeltoken(ev[1], ev[2])
                self.long_memory(ev[1])
            elif ev[0] == "height":
                self.base_height.append(ev[1])
            elif ev[0] == "skipped":
                self._log(f"move failed: {ev[1]}")

    def _explorer(self):
        if self.Env is None:
            raise RuntimeError("this call drives a simulator: construct VoxelTokenMemory(..., env=<NavEnv-like object>), or feed "
                               "frames through obs2voxeltoken() / ingest_frames() / dataset.create_memory_for_dataset()")
        from .dataset import EnvExplorer
        return EnvExplorer(self.Env)

    def excute(self, obs, actions):
        """memory_2.py:1086-1101 (the reference's spelling): step the simulator, ingest every frame -> last observation."""
        ex = self._explorer()
        ex.last_obs = obs
        self._consume(ex.frames(actions))
        return ex.last_obs

    def exploring_create_memory(self):
        """memory_2.py:1104-1145: random goals with a 360 degree sweep at each, final flush of the token cache, save."""
        ex = self._explorer()
        self.initial_memory()
        self.init_height = self.Env.agent.get_state().position[1]
        with self.prefetched_sampling():
            self._consume(ex.tour(self.cfg.random_move_num, self.cfg.turn_left))
        if self.feature_mode == "exact":
            self.update_memory_dist_base()
        self.save_memory()

    def create_memory(self):
        raise NotImplementedError("keyboard-driven exploration (memory_2.py:1027-1083) is a UI loop over the simulator's viewer "
                                  "(out of scope, SURVEY.md §2 #9); use exploring_create_memory() with an injected env, or feed "
                                  "frames through obs2voxeltoken() / ingest_frames() / dataset.create_memory_for_dataset()")

    def explore_entire_space(self, max_iterations=30):
        """memory_2.py:1347-1391: look around, find the frontier clusters of the top-down map (frontier.hip), walk to the most
        informative one, repeat."""
        ex = self._explorer()
        self.min_cluster_size, self.ig_radius = 10, 5
        self.initial_memory()
        for _ in range(max_iterations):
            self._consume(ex.frames(ex.sweep(self.cfg.turn_left)))
            navigable = self.build_navigable_mask()
            frontiers = self.find_frontiers(navigable)
            clusters = self.cluster_frontiers(frontiers) if frontiers else []
            target = self.select_best_cluster_center_by_ig(clusters) if clusters else None
            if target is None:
                break
            self.update_frontier_map(frontiers, clusters, target, navigable)
            path, _goal = self.Env.move2point(self.Env.get_random_navigable_point_near(self.grid2loc_2d(target[0], target[1])))
            self._consume(ex.frames(path))

    # ---- FrontierExplorer (memory_2.py:1147-1418) -----------------------------------------------------------------
    # The per-cell Python loops of the reference run as HIP kernels over the resident top-down map
    # (csrc/frontier.hip); the simulator only enters through Env.plnner.pathfinder.is_navigable.
    def grid2loc_2d(self, x, y):
        """memory_2.py:1148-1158."""
        ix, iz, iy = self.Env.original_state.position
        return np.array([ix + (y - self.gs // 2) * self.cs, iz, iy + (x - self.gs // 2) * self.cs])

    def loc2grid_2d(self, x_base, y_base):
        """memory_2.py:1160-1163."""
        return int(self.gs / 2 - int(x_base / self.cs)), int(self.gs / 2 - int(y_base / self.cs))

    def in_bounds(self, x, y):
        return 0 <= x < self.gs and 0 <= y < self.gs

    def is_unknown(self, x, y):
        """memory_2.py:1165."""
        return not bool(self.engine.frontier_mask()[x, y] & 1)

    def is_known(self, x, y):
        return not self.is_unknown(x, y)

    def is_navigabale(self, x, y):
        """memory_2.py:1171 (the reference's spelling)."""
        return self.Env.plnner.pathfinder.is_navigable(self.grid2loc_2d(x, y))

    def build_navigable_mask(self):
        """memory_2.py:1174-1185: known cells the simulator calls navigable (only known cells are asked)."""
        known = (self.engine.frontier_mask() & 1).astype(bool)
        mask = np.zeros((self.gs, self.gs), dtype=bool)
        for x, y in np.argwhere(known):
            mask[x, y] = bool(self.is_navigabale(int(x), int(y)))
        return mask

    def find_frontiers(self, navigable_mask):
        """memory_2.py:1187-1209 -> [(x, y), ...] row-major."""
        m = self.engine.frontier_mask(navigable_mask)
        return [(int(x), int(y)) for x, y in np.argwhere(m & 2)]

    def _frontier_clusters(self, frontiers):
        fr = np.zeros((self.gs, self.gs), np.uint8)
        if len(frontiers):
            f = np.asarray(frontiers, np.int64).reshape(-1, 2)
            fr[f[:, 0], f[:, 1]] = 1
        return self.engine.frontier_clusters(fr, getattr(self, "min_cluster_size", 10), getattr(self, "ig_radius", 5),
                                             max_clusters=self.gs * self.gs)

    def cluster_frontiers(self, frontiers):
        """memory_2.py:1211-1249 -> list of clusters (lists of (x, y)) with >= min_cluster_size cells, in the reference's
        order.  Cells inside a cluster are listed row-major (the reference lists them in BFS order; every consumer
        is order-free: mean, membership)."""
        if not frontiers:
            return []
        r = self._frontier_clusters(frontiers)
        self._last_clusters = r
        lab = r["labels"]
        cells = np.argwhere(lab >= 0)
        out = [[] for _ in range(r["n"])]
        for x, y in cells:
            out[lab[x, y]].append((int(x), int(y)))
        return out

    def compute_cluster_center(self, cluster):
        """memory_2.py:1252-1258."""
        return (sum(p[0] for p in cluster) / len(cluster), sum(p[1] for p in cluster) / len(cluster))

    def compute_information_gain(self, center_x, center_y):
        """memory_2.py:1260-1280: unknown cells within ig_radius (Chebyshev) of the rounded centre."""
        known = (self.engine.frontier_mask() & 1).astype(bool)
        cx, cy, r = int(round(center_x)), int(round(center_y)), getattr(self, "ig_radius", 5)
        win = known[max(cx - r, 0):max(cx + r + 1, 0), max(cy - r, 0):max(cy + r + 1, 0)]
        return float(win.size - int(win.sum()))

    def select_best_cluster_center_by_ig(self, frontier_clusters):
        """memory_2.py:1282-1311: centre of the first cluster with the strictly largest gain > 0, else None."""
        if not frontier_clusters:
            return None
        fr = [c for cl in frontier_clusters for c in cl]
        r = self._frontier_clusters(fr)
        # clusters handed in may be a subset / regrouping of the device clusters: match them by first cell
        if r["n"] == len(frontier_clusters) and all(tuple(r["first"][k]) == min(frontier_clusters[k]) for k in range(r["n"])):
            return None if r["best"] < 0 else (float(r["centers"][r["best"], 0]), float(r["centers"][r["best"], 1]))
        best, best_ig = None, 0.0
        for cl in frontier_clusters:
            cx, cy = self.compute_cluster_center(cl)
            ig = self.compute_information_gain(cx, cy)
            if ig > best_ig:
                best_ig, best = ig, (cx, cy)
        return best

    def update_frontier_map(self, frontiers, frontier_clusters, target_center_map, navigable_mask=None):
        """memory_2.py:1313-1344: black unknown, white known + navigable, grey known, red frontier cells, green target
        disc (radius 5, drawn like cv2.circle(img, (ty, tx), 5, ..., -1))."""
        known = (self.engine.frontier_mask() & 1).astype(bool)
        if navigable_mask is None:
            navigable_mask = self.build_navigable_mask()
        img = np.zeros((self.gs, self.gs, 3), np.uint8)
        img[known] = (100, 100, 100)
        img[known & np.asarray(navigable_mask, bool)] = (255, 255, 255)
        for fx, fy in frontiers:
            img[fx, fy] = (255, 0, 0)
        if target_center_map is not None:
            tx, ty = int(round(target_center_map[0])), int(round(target_center_map[1]))
            if 0 <= tx < self.gs and 0 <= ty < self.gs:
                xx, yy = np.ogrid[0:self.gs, 0:self.gs]
                img[(xx - tx) ** 2 + (yy - ty) ** 2 <= 25] = (0, 255, 0)
        self.FrontierMap = img

    # ---- BASELINE.json vocabulary (north_star names the entry points Memory.update_* / Memory.localize) -------------
    def update_from_observation(self, obs, pose):
        """Alias of obs2voxeltoken (memory_2.py:842)."""
        return self.obs2voxeltoken(obs, pose)

    def update_from_frames(self, rgb, depth, poses, tokens=None):
        """Alias of ingest_frames (batched form of obs2voxeltoken)."""
        return self.ingest_frames(rgb, depth, poses, tokens)

    def localize(self, prompt, K=100, **kw):
        """Alias of voxel_localized (memory_2.py:563)."""
        return self.voxel_localized(prompt, K=K, **kw)


Memory = VoxelTokenMemory
