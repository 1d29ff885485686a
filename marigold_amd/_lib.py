"""ctypes binding of libmarigold_hip.so (C ABI in include/marigold_hip.h).

The product path has NO fallback: if the HIP library is missing or does not export the ABI
this module raises, loudly.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``make -C marigold_amd/csrc``).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MARIGOLD_HIP_LIB") or os.path.join(_HERE, "libmarigold_hip.so")   # (override: same-box A/B of two builds)
ABI_VERSION = 4

# enum mg_op_kind
OP_IGEMM, OP_GN_STATS, OP_GN_FINALIZE, OP_GN_APPLY = 1, 2, 3, 4
OP_FLASH_ATTN64, OP_SOFTMAX_ROWS = 6, 7
OP_GN_SLAB = 9
OP_ROWGEMM = 10
OP_FLASH_ATTN512 = 11
RG_BF16, RG_GEGLU, RG_QKV, RG_XATTN = 0, 1, 2, 3
OP_SCHED_STEP = 12
OP_LINEAR_SMALL_M, OP_LATENT_1X1, OP_POST_NCHW, OP_IM2COL_SMALL = 13, 14, 15, 16
OP_CONV3X3 = 17
OP_CONV3X3_HEAD = 18
OP_ENS_DEPTH_STATS, OP_ENS_DEPTH_MEDIAN, OP_ENS_DEPTH_NORM, OP_ENS_NORMALS = 20, 21, 22, 23
OP_RESIZE = 24
OP_COLORIZE = 25
OP_EVAL_DEPTH_LS, OP_EVAL_DEPTH_METRICS, OP_EVAL_NORMALS = 26, 27, 28
EVAL_WS_BYTES = 128 * 1024   # MG_EVAL_WS_BYTES
EVAL_ALIGN = {None: 0, "least_square": 1, "least_square_disparity": 2}   # MG_EVAL_ALIGN_*
OP_MEMSET, OP_COPY = 30, 31
OP_IIDSCORE_PREP, OP_IIDSCORE_PSNR, OP_IIDSCORE_SSIM = 32, 33, 34
OP_IID_VIS = 35
OP_RGB_PREP, OP_NORMALS_VIS = 5, 8   # the I/O stages: free numbers below the last kind
OP_RANDN = 29   # the native noise generator: likewise
OP_ENS_IID = 19   # the intrinsic-image ensemble: the free number below the first ensembling kind
IID_VIS_PARTS = 128   # MG_IID_VIS_PARTS
IID_GAMMA = {None: 0, 2.2: 1, 1.0 / 2.2: 2, (2.2, 1.0 / 2.2): 3}   # MG_IID_GAMMA_*
IID_METRICS = {"psnr": 1, "ssim": 2}   # MG_IID_*


def iid_gamma_mode(gamma):
    """MG_IID_GAMMA_* of ``gamma``: None, 2.2, 1 / 2.2 or the pair (2.2, 1 / 2.2); a number within 1e-3 (relative) of 2.2 or 1 / 2.2
    names that conversion (0.4545, numpy.float32(2.2)) - the kernels raise to the exact exponents."""
    if gamma is None:
        return 0
    if isinstance(gamma, (list, tuple)):
        modes = [iid_gamma_mode(g) for g in gamma]
        if modes in ([1], [2]):
            return modes[0]
        if modes == [1, 2]:
            return 3
        raise ValueError(f"gamma {gamma!r}: only (2.2, 1 / 2.2), in that order, is a pair the scorer applies")
    for mode, exponent in ((1, 2.2), (2, 1.0 / 2.2)):
        if abs(float(gamma) - exponent) <= 1e-3 * exponent:
            return mode
    raise ValueError(f"gamma {gamma!r} is not None, 2.2, 1 / 2.2 or (2.2, 1 / 2.2)")
EPI_BF16, EPI_GEGLU, EPI_F32, EPI_SOFTMAX2, EPI_XATTN2 = 0, 1, 2, 3, 4
POST_NONE, POST_DEPTH, POST_NORMALS, POST_UNIT, POST_SCHED = 0, 1, 2, 3, 4

# Field names of every kind: kind -> (enumerator prefix, {array: names in slot order}) - the mirror of the
# MG_<KIND>_<I|F|P|L>_<NAME> enumerators of include/marigold_hip.h (lower case here; the position is the slot).
# tests/test_host.py compares the two; ops.py builds and reads every kind by these names.
FIELDS = {
    OP_IGEMM: ("IGEMM", dict(
        i=("b", "h", "w", "cin", "ho", "wo", "n", "taps", "stride", "pad", "hu", "wu", "epi", "ldo", "trans_from", "batch_z", "ldr",
           "lda", "ldt", "variant", "ldw", "rowvec_bcast", "n_alg", "k_alg", "c0", "lda1", "trans_perm", "sm_cols", "c2",
           "tickets_lo", "tickets_hi", "splits", "cx", "cx0", "ldx0", "ldx1"),
        f=("scale", "ln_eps", "sm_scale"),
        p=("a", "wt", "out", "bias", "rowvec", "residual", "out2", "a1", "ln_out", "ln_in", "ln_g", "ln_c", "x0", "x1", "splitk_ws"),
        l=("sa", "sw", "so", "sr"))),
    OP_CONV3X3: ("CONV3X3", dict(
        i=("b", "h", "w", "c0", "c1", "n", "subpix", "silu", "lda0", "lda1", "ldo", "ldr", "ldw", "rowvec_bcast", "variant", "gn_cpg",
           "gn_slots"),
        p=("a0", "wt", "out", "bias", "rowvec", "residual", "a1", "ss", "gn_part"),
        l=("sw",))),
    OP_ROWGEMM: ("ROWGEMM", dict(
        i=("m", "k", "n", "ldx", "ldo", "ldr", "form", "tokens", "ldt", "trans_from", "waves", "sm_cols", "nsplit"),
        f=("ln_eps", "sm_scale"),
        p=("x", "wp", "out", "residual", "ln_in", "ln_out", "vt", "gn_ss", "dbg", "xattn", "xout"))),
    OP_FLASH_ATTN64: ("FLASH64", dict(
        i=("b", "heads", "ntok", "ldq", "ldo", "ldvt", "variant", "vt_perm", "ws_kb", "split"),
        f=("scale", "redo_thr"),
        p=("q", "k", "vt", "o", "dbg", "ws"),
        l=("sq", "sk", "svt", "so"))),
    OP_RGB_PREP: ("RGB_PREP", dict(
        i=("hin", "win", "hout", "wout", "mode", "hwc", "out16", "reciprocal"),
        p=("src", "dst", "tmp"))),
    OP_NORMALS_VIS: ("NORMALS_VIS", dict(
        i=("h", "w"),
        p=("pred", "out"))),
    OP_RANDN: ("RANDN", dict(
        i=("mode", "out16"),
        p=("dst",),
        l=("n", "offset", "seed", "stream"))),
    OP_ENS_IID: ("ENS_IID", dict(
        i=("e", "reduction"),
        p=("preds", "pred", "unc"),
        l=("n",))),
    OP_GN_STATS: ("GN_STATS", dict(
        i=("b", "hw", "c", "chunks", "ctot", "coff", "groups", "slot0", "slots", "c1"),
        f=("eps",),
        p=("x", "partials", "gamma", "beta", "ss", "counters", "x1"))),
    OP_GN_FINALIZE: ("GN_FINALIZE", dict(
        i=("b", "c", "groups", "slots", "hw"),
        f=("eps",),
        p=("partials", "gamma", "beta", "ss"))),
    OP_GN_APPLY: ("GN_APPLY", dict(
        i=("b", "hw", "c", "silu", "c0"),
        p=("x", "ss", "out", "x1"))),
    OP_GN_SLAB: ("GN_SLAB", dict(
        i=("b", "hw", "c", "c0", "groups", "silu"),
        f=("eps",),
        p=("x0", "x1", "out", "gamma", "beta", "ss"))),
    OP_FLASH_ATTN512: ("FLASH_ATTN512", dict(
        i=("b", "ntok", "ldq", "ldo", "ldvt"),
        f=("scale",),
        p=("q", "k", "vt", "o"),
        l=("sq", "sk", "svt", "so"))),
    OP_SOFTMAX_ROWS: ("SOFTMAX_ROWS", dict(
        i=("r", "ncols", "lds", "ldp"),
        p=("scores", "probs"))),
    OP_SCHED_STEP: ("SCHED_STEP", dict(
        f=("cx", "cm", "cn"),
        p=("x", "model_out", "noise", "out"),
        l=("n",))),
    OP_LINEAR_SMALL_M: ("LINEAR_SMALL_M", dict(
        i=("m", "n", "k", "act_in", "act_out", "ldo"),
        p=("x", "w", "bias", "out"))),
    OP_LATENT_1X1: ("LATENT_1X1", dict(
        i=("b", "ci", "co", "hw"),
        f=("scale",),
        p=("x", "w", "bias", "out"))),
    OP_POST_NCHW: ("POST_NCHW", dict(
        i=("b", "hw", "cout", "ldi", "post"),
        f=("scale", "cx", "cm", "cn"),
        p=("x", "out", "noise"))),
    OP_IM2COL_SMALL: ("IM2COL_SMALL", dict(
        i=("b", "h", "w", "c0", "c1", "kp", "src0_broadcast", "members_per_src0"),
        p=("src0", "src1", "out"))),
    OP_CONV3X3_HEAD: ("CONV3X3_HEAD", dict(
        i=("b", "h", "w", "c", "cout", "ldo", "silu"),
        p=("x", "ss", "wt", "bias", "out"))),
    OP_ENS_DEPTH_STATS: ("ENS_DEPTH_STATS", dict(
        i=("e",),
        p=("d", "scratch", "out"),
        l=("hw",))),
    OP_ENS_DEPTH_MEDIAN: ("ENS_DEPTH_MEDIAN", dict(
        i=("e", "reduction", "has_shift"),
        p=("d", "st", "med", "mad", "minmax", "scratch"),
        l=("hw",))),
    OP_ENS_DEPTH_NORM: ("ENS_DEPTH_NORM", dict(
        i=("shift_invariant",),
        p=("med", "mad", "minmax"),
        l=("hw",))),
    OP_ENS_NORMALS: ("ENS_NORMALS", dict(
        i=("e", "reduction"),
        p=("normals", "out", "unc"),
        l=("hw",))),
    OP_RESIZE: ("RESIZE", dict(
        i=("planes", "hin", "win", "hout", "wout", "mode", "u8"),
        p=("src", "dst", "tmp"))),
    OP_COLORIZE: ("COLORIZE", dict(
        f=("min_depth", "max_depth"),
        p=("depth", "lut", "out", "clipped", "u16"),
        l=("n",))),
    OP_EVAL_DEPTH_LS: ("EVAL_DEPTH_LS", dict(
        i=("h", "w", "disparity", "fit_w"),
        f=("inv_factor",),
        p=("pred", "gt", "mask", "out", "scratch"))),
    OP_EVAL_DEPTH_METRICS: ("EVAL_DEPTH_METRICS", dict(
        i=("h", "w", "disparity", "clip_min", "clip_max"),
        f=("min_depth", "max_depth"),
        p=("pred", "gt", "mask", "sums", "out", "scratch"))),
    OP_EVAL_NORMALS: ("EVAL_NORMALS", dict(
        i=("masked",),
        p=("pred", "gt", "out", "err", "ws"),
        l=("hw",))),
    OP_MEMSET: ("MEMSET", dict(
        i=("value",),
        p=("dst",),
        l=("bytes",))),
    OP_COPY: ("COPY", dict(
        p=("src", "dst"),
        l=("bytes",))),
    OP_IIDSCORE_PREP: ("IIDSCORE_PREP", dict(
        i=("h", "w", "gamma"),
        p=("pred", "gt", "mask", "out", "ws"))),
    OP_IIDSCORE_PSNR: ("IIDSCORE_PSNR", dict(
        i=("h", "w", "gamma", "up_to_scale", "write_psnr"),
        p=("pred", "gt", "mask", "out", "ws"))),
    OP_IIDSCORE_SSIM: ("IIDSCORE_SSIM", dict(
        i=("h", "w", "gamma", "up_to_scale"),
        p=("pred", "gt", "mask", "out", "ws"))),
    OP_IID_VIS: ("IID_VIS", dict(
        i=("n", "h", "w", "linear_bits", "up_to_scale_bits"),
        p=("pred", "out", "ws"))),
}

OP_NAMES = {v: k[3:].lower() for k, v in list(globals().items()) if k.startswith("OP_")}

EXPORTS = [
    "mg_abi_version", "mg_operand_bits", "mg_last_error", "mg_init", "mg_geglu_interleave", "mg_device_info", "mg_launch",
    "mg_program_create", "mg_program_num_ops", "mg_program_run", "mg_program_validate", "mg_program_run_range",
    "mg_program_capture", "mg_program_profile", "mg_program_destroy", "mg_conv2d_igemm", "mg_conv3x3", "mg_conv3x3_gn_slots", "mg_flash4w_plan_test",
    "mg_sched_step", "mg_ensemble_normals", "mg_ens_align_cost_grad", "mg_bfgs_minimize", "mg_ens_align_minimize", "mg_event_create", "mg_event_record",
    "mg_event_elapsed_ms", "mg_event_destroy", "mg_clock_probe", "mg_debug_read_workspace",
    "mg_model_load", "mg_model_destroy", "mg_model_info", "mg_model_device_bytes", "mg_model_validate", "mg_model_vae_encode",
    "mg_model_denoise", "mg_model_vae_decode", "mg_ensemble_depth", "mg_eval_depth", "mg_eval_normals", "mg_eval_iid",
    "mg_rgb_prepare", "mg_normals_visualize",
    "mg_randn", "mg_resize", "mg_colorize", "mg_iid_visualize", "mg_model_predict",
    "mg_ensemble_iid", "mg_model_predict_iid",
    "mg_depth_visualize", "mg_normals_finish", "mg_model_predict_out", "mg_model_predict_many",
    "mg_lpips_workspace_bytes", "mg_eval_iid_lpips",
    "mg_model_num_configs", "mg_model_config_info", "mg_model_find_config", "mg_model_select", "mg_processed_size",
    "mg_model_shared_bytes", "mg_model_replica",
    "mg_latent_carry", "mg_model_seq_reset", "mg_model_predict_next",
    "mg_tiny_vae_workspace_bytes", "mg_tiny_vae_encode", "mg_tiny_vae_decode", "mg_tiny_conv3x3",
    "mg_model_scratch_fill",
    "mg_tile_plan", "mg_tiles_workspace_bytes", "mg_tile_fit", "mg_tile_blend",
    "mg_tile_crop", "mg_model_predict_tiled",
    "mg_guided_upsample",
    "mg_depth_align_workspace_bytes", "mg_depth_align_fit", "mg_depth_align_apply",
    "mg_depth_normals", "mg_depth_points_workspace_bytes", "mg_depth_points",
    "mg_depth_mesh_workspace_bytes", "mg_depth_mesh",
    "mg_depth_view_workspace_bytes", "mg_depth_view",
    "mg_depth_focus_workspace_bytes", "mg_depth_focus",
]


class MgPredictOpts(ctypes.Structure):
    """mg_predict_opts; the defaults are MG_PREDICT_OPTS_DEFAULT (the reference's)."""
    _fields_ = [("scale_invariant", ctypes.c_int), ("shift_invariant", ctypes.c_int), ("reduction", ctypes.c_int), ("max_iter", ctypes.c_int),
                ("max_res", ctypes.c_int), ("normals_reduction", ctypes.c_int), ("regularizer_strength", ctypes.c_double), ("tol", ctypes.c_double)]

    def __init__(self, scale_invariant=1, shift_invariant=1, reduction=0, max_iter=50, max_res=1024, normals_reduction=0,
                 regularizer_strength=0.02, tol=1e-6):
        super().__init__(scale_invariant, shift_invariant, reduction, max_iter, max_res, normals_reduction, regularizer_strength, tol)


class MgIidOpts(ctypes.Structure):
    """mg_iid_opts; the defaults are MG_IID_OPTS_DEFAULT (the median, every target in sRGB space, the model's output size)."""
    _fields_ = [("reduction", ctypes.c_int), ("linear_bits", ctypes.c_int), ("up_to_scale_bits", ctypes.c_int), ("out_h", ctypes.c_int),
                ("out_w", ctypes.c_int), ("out_mode", ctypes.c_int)]


class MgOutputOpts(ctypes.Structure):
    """mg_output_opts; the defaults are MG_OUTPUT_OPTS_DEFAULT (the model's output size, no colour table).  ``lut256x3``: the DEVICE
    address of the colour map's 256 x 3 uint8 table."""
    _fields_ = [("out_h", ctypes.c_int), ("out_w", ctypes.c_int), ("out_mode", ctypes.c_int), ("lut256x3", ctypes.c_void_p)]


class MgTiledOpts(ctypes.Structure):
    """mg_tiled_opts: the configurations of the model image (``mg_model_find_config``) - the guide's, the tiles' and, or -1, the short
    last group's - and the minimum overlap along y and x."""
    _fields_ = [("guide_config", ctypes.c_int), ("tile_config", ctypes.c_int), ("overlap_y", ctypes.c_int), ("overlap_x", ctypes.c_int),
                ("tail_config", ctypes.c_int)]

    def __init__(self, guide_config=0, tile_config=0, overlap_y=0, overlap_x=0, tail_config=-1):
        super().__init__(guide_config, tile_config, overlap_y, overlap_x, tail_config)


class MgLpipsNet(ctypes.Structure):
    """mg_lpips_net: DEVICE addresses of the fp32 weights of the five layers, packed as the header documents."""
    _fields_ = [("conv_w", ctypes.c_void_p * 5), ("conv_b", ctypes.c_void_p * 5), ("lin_w", ctypes.c_void_p * 5)]


TILE_MAX_PER_AXIS = 32   # MG_TILE_MAX_PER_AXIS
ALIGN_MAX_ITERS = 32   # MG_ALIGN_MAX_ITERS
ALIGN_START_GIVEN, ALIGN_START_LS = 0, 1   # MG_ALIGN_START_*
NORMALS_FRAME = {"camera": 0, "marigold": 1}   # MG_NORMALS_FRAME_*
VIEW_MAX_SPAN, VIEW_MAX_FILL = 64, 64   # MG_VIEW_MAX_SPAN, MG_VIEW_MAX_FILL
FOCUS_MAX_RADIUS = 32   # MG_FOCUS_MAX_RADIUS
FOCUS_SPACE = {"lens": 0, "linear": 1}   # MG_FOCUS_SPACE_*
TINY_VAE_LAYERS = 33   # MG_TINY_VAE_LAYERS: the 64 -> 64 layers of either half
# enum mg_cfg: the configuration words of a model image (mg_model_info), position = word; "pictures" is written 0 for 1.  An image
# holds CFG_WORDS of them: what lies behind the named ones is reserved, written 0
CFG = ("members", "height", "width", "latent_h", "latent_w", "steps", "channels", "post", "step_noises", "op_bytes", "modalities",
       "out_h", "out_w", "pictures", "vae")
CFG_WORDS = 16
VAE_KL, VAE_TINY = 0, 1   # MG_VAE_*: the word "vae"


class MgTinyVae(ctypes.Structure):
    """mg_tiny_vae: DEVICE addresses of the packed weights and fp32 biases of both halves, in the layout the header documents."""
    _fields_ = [(f"{half}_{name}", ctype) for half in ("enc", "dec") for name, ctype in (
        ("in_w", ctypes.c_void_p), ("in_b", ctypes.c_void_p), ("w", ctypes.c_void_p * TINY_VAE_LAYERS),
        ("b", ctypes.c_void_p * TINY_VAE_LAYERS), ("out_w", ctypes.c_void_p), ("out_b", ctypes.c_void_p))]


class MgOp(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("i", ctypes.c_int32 * 40), ("f", ctypes.c_float * 8),
                ("p", ctypes.c_void_p * 16), ("l", ctypes.c_int64 * 4)]


class MarigoldHipError(RuntimeError):
    pass


# The fp16-operand twin (csrc/Makefile: OPERAND_F16=1, same sources, same ABI): what the engine modules load for
# torch_dtype=torch.float16 (the reference's --fp16, script/depth/run.py:203-211).  Its own globals, its own mg_init.
LIB_PATH_F16 = os.environ.get("MARIGOLD_HIP_LIB_F16") or os.path.join(_HERE, "libmarigold_hip_f16.so")

_libs = {}


def load(f16=False):
    """Load the shared library (no GPU needed) and check that every ABI symbol is exported.  ``f16``: the fp16-operand build."""
    key = bool(f16)
    if key in _libs:
        return _libs[key]
    path = LIB_PATH_F16 if key else LIB_PATH
    if not os.path.exists(path):
        raise MarigoldHipError(
            f"{path} not found: the HIP engine is not built. Run __graft_entry__.build() "
            f"(make -C marigold_amd/csrc). There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    missing = [s for s in EXPORTS if not hasattr(lib, s)]
    if missing:
        raise MarigoldHipError(f"{path} lacks ABI symbols: {missing}")
    lib.mg_last_error.restype = ctypes.c_char_p
    lib.mg_launch.argtypes = [ctypes.POINTER(MgOp), ctypes.c_void_p]
    lib.mg_geglu_interleave.restype = ctypes.c_int
    lib.mg_conv2d_igemm.argtypes = [ctypes.POINTER(MgOp), ctypes.c_void_p]
    lib.mg_conv3x3.argtypes = [ctypes.POINTER(MgOp), ctypes.c_void_p]
    lib.mg_conv3x3_gn_slots.argtypes = [ctypes.POINTER(MgOp)]
    lib.mg_conv3x3_gn_slots.restype = ctypes.c_int
    lib.mg_flash4w_plan_test.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint)]
    lib.mg_program_create.restype = ctypes.c_void_p
    lib.mg_program_create.argtypes = [ctypes.POINTER(MgOp), ctypes.c_int]
    lib.mg_program_num_ops.argtypes = [ctypes.c_void_p]
    lib.mg_ens_align_cost_grad.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 7
    lib.mg_bfgs_minimize.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_ens_align_minimize.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_program_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_program_validate.argtypes = [ctypes.c_void_p]
    lib.mg_program_run_range.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.mg_program_capture.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_program_profile.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.mg_program_destroy.argtypes = [ctypes.c_void_p]
    lib.mg_program_destroy.restype = None
    lib.mg_sched_step.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_float] * 3 + [ctypes.c_void_p]
    lib.mg_ensemble_normals.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    lib.mg_device_info.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_int64), ctypes.c_char_p, ctypes.c_int]
    lib.mg_clock_probe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.mg_debug_read_workspace.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.mg_model_load.restype = ctypes.c_void_p
    lib.mg_model_load.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.mg_model_destroy.argtypes = [ctypes.c_void_p]
    lib.mg_model_destroy.restype = None
    lib.mg_model_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    lib.mg_model_device_bytes.argtypes = [ctypes.c_void_p]
    lib.mg_model_device_bytes.restype = ctypes.c_longlong
    lib.mg_model_validate.argtypes = [ctypes.c_void_p]
    lib.mg_model_vae_encode.argtypes = [ctypes.c_void_p] * 4
    lib.mg_model_denoise.argtypes = [ctypes.c_void_p] * 5
    lib.mg_model_vae_decode.argtypes = [ctypes.c_void_p] * 4
    lib.mg_ensemble_depth.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                      ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_eval_depth.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_double] * 2 + [ctypes.c_void_p] * 3
    lib.mg_eval_normals.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 4
    lib.mg_eval_iid.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3
    lib.mg_lpips_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.mg_lpips_workspace_bytes.restype = ctypes.c_longlong
    lib.mg_eval_iid_lpips.argtypes = [ctypes.POINTER(MgLpipsNet)] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + \
        [ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_tiny_vae_workspace_bytes.argtypes = [ctypes.c_int] * 4
    lib.mg_tiny_vae_workspace_bytes.restype = ctypes.c_longlong
    lib.mg_tiny_vae_encode.argtypes = [ctypes.POINTER(MgTinyVae)] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_tiny_vae_decode.argtypes = [ctypes.POINTER(MgTinyVae)] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + \
        [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_tiny_conv3x3.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    lib.mg_rgb_prepare.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    lib.mg_normals_visualize.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_randn.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.mg_resize.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    lib.mg_colorize.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
    lib.mg_iid_visualize.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    lib.mg_model_predict.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_uint64, ctypes.POINTER(MgPredictOpts)] + [ctypes.c_void_p] * 4
    lib.mg_ensemble_iid.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_model_predict_iid.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_uint64, ctypes.POINTER(MgIidOpts)] + [ctypes.c_void_p] * 4
    lib.mg_depth_visualize.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int64] + [ctypes.c_void_p] * 4
    lib.mg_normals_finish.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    lib.mg_model_predict_out.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_uint64, ctypes.POINTER(MgPredictOpts),
                                                                                       ctypes.POINTER(MgOutputOpts)] + [ctypes.c_void_p] * 6
    lib.mg_model_predict_many.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)] + [ctypes.c_int] * 5 + \
        [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(MgPredictOpts), ctypes.POINTER(MgOutputOpts)] + [ctypes.c_void_p] * 6
    lib.mg_latent_carry.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p]
    lib.mg_model_seq_reset.argtypes = [ctypes.c_void_p]
    lib.mg_tile_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.mg_tiles_workspace_bytes.argtypes = [ctypes.c_int] * 3
    lib.mg_tiles_workspace_bytes.restype = ctypes.c_longlong
    _grid = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_int]   # ystarts, ny, xstarts, nx, Hw, Ww
    lib.mg_tile_fit.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + _grid + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + \
        [ctypes.c_void_p] * 3 + [ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_tile_blend.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + _grid + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                                                 ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_tile_crop.argtypes = [ctypes.c_void_p] + _grid[4:] + [ctypes.c_int] * 3 + _grid[:4] + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_model_predict_tiled.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_uint64, ctypes.POINTER(MgTiledOpts),
                                                                                         ctypes.POINTER(MgPredictOpts),
                                                                                         ctypes.POINTER(MgOutputOpts)] + [ctypes.c_void_p] * 7
    lib.mg_guided_upsample.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + \
        [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_depth_align_workspace_bytes.argtypes = [ctypes.c_longlong]
    lib.mg_depth_align_workspace_bytes.restype = ctypes.c_longlong
    lib.mg_depth_align_fit.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_longlong] + [ctypes.c_int] * 3 + [ctypes.c_double] * 3 + \
        [ctypes.c_void_p] * 3 + [ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_depth_align_apply.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_depth_normals.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_double] * 7 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    lib.mg_depth_points_workspace_bytes.argtypes = [ctypes.c_longlong]
    lib.mg_depth_points_workspace_bytes.restype = ctypes.c_longlong
    lib.mg_depth_points.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 2 + \
        [ctypes.c_double] * 7 + [ctypes.c_int, ctypes.c_longlong] + [ctypes.c_void_p] * 6 + [ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_depth_mesh_workspace_bytes.argtypes = [ctypes.c_longlong]
    lib.mg_depth_mesh_workspace_bytes.restype = ctypes.c_longlong
    lib.mg_depth_mesh.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 2 + \
        [ctypes.c_double] * 7 + [ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong] + [ctypes.c_void_p] * 7 + [ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_depth_view_workspace_bytes.argtypes = [ctypes.c_longlong]
    lib.mg_depth_view_workspace_bytes.restype = ctypes.c_longlong
    lib.mg_depth_view.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 2 + \
        [ctypes.c_double] * 7 + [ctypes.c_void_p] + [ctypes.c_double] * 4 + [ctypes.c_int] * 2 + [ctypes.c_double, ctypes.c_int] + \
        [ctypes.c_void_p] * 6 + [ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_depth_focus_workspace_bytes.argtypes = [ctypes.c_longlong]
    lib.mg_depth_focus_workspace_bytes.restype = ctypes.c_longlong
    lib.mg_depth_focus.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 2 + \
        [ctypes.c_double] * 2 + [ctypes.c_int, ctypes.c_double] + [ctypes.c_int] * 3 + [ctypes.c_double] + [ctypes.c_void_p] * 5 + \
        [ctypes.c_longlong, ctypes.c_void_p]
    lib.mg_model_scratch_fill.argtypes =[ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.mg_model_predict_next.argtypes = lib.mg_model_predict_out.argtypes + [ctypes.c_float]
    lib.mg_model_num_configs.argtypes = [ctypes.c_void_p]
    lib.mg_model_config_info.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.mg_model_find_config.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5
    lib.mg_model_select.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.mg_processed_size.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 2
    lib.mg_model_shared_bytes.argtypes = [ctypes.c_void_p]
    lib.mg_model_shared_bytes.restype = ctypes.c_longlong
    lib.mg_model_replica.argtypes = [ctypes.c_void_p]
    lib.mg_model_replica.restype = ctypes.c_void_p
    lib.mg_event_create.restype = ctypes.c_void_p
    lib.mg_event_record.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mg_event_elapsed_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.mg_event_destroy.argtypes = [ctypes.c_void_p]
    lib.mg_event_destroy.restype = None
    lib.mg_operand_bits.restype = ctypes.c_int
    if lib.mg_abi_version() != ABI_VERSION:
        raise MarigoldHipError(f"ABI version mismatch: library {lib.mg_abi_version()}, binding {ABI_VERSION}")
    if bool(lib.mg_operand_bits() & 1) != key:
        raise MarigoldHipError(f"{path} is the {'fp16' if lib.mg_operand_bits() & 1 else 'bf16'}-operand build")
    lib._mg_f16 = key
    _libs[key] = lib
    return lib


def check(rc, what="libmarigold_hip", lib=None):
    if rc != 0:
        msgs = [(lib or l_).mg_last_error().decode(errors="replace") for l_ in ([lib] if lib is not None else list(_libs.values()) or [load()])]
        raise MarigoldHipError(f"{what}: {' | '.join(m for m in msgs if m) or 'error'}")


_inited = set()


def init(device_index=0, f16=False):
    """Bind the library to a GPU (one process drives one GPU)."""
    lib = load(f16)
    if (device_index, bool(f16)) not in _inited:
        check(lib.mg_init(int(device_index)), "mg_init", lib)
        _inited.add((device_index, bool(f16)))
    return lib
