"""Multi-image inference CLI with the reference's flags and on-disk formats
(script/depth/run.py:54-135 flags, :165-171 output folders, :270-292 files; script/normals/run.py is
the same minus ``--color_map``):

  depth   : <out>/depth_npy/<name>_depth.npy      float32 [H,W] in [0,1]
            <out>/depth_bw/<name>_depth.png        16-bit PNG, value * 65535
            <out>/depth_colored/<name>_depth_colored.png
            <out>/depth_points/<name>_points.ply   with --save_points (an extension): the map as a coloured point cloud, binary PLY
            <out>/depth_mesh/<name>_mesh.ply       with --save_mesh (an extension): the map as a coloured triangle mesh, binary PLY
            <out>/depth_stereo/<name>_stereo.png   with --save_stereo (an extension): the picture from two eyes, left beside right
            <out>/depth_refocus/<name>_refocus.png with --save_refocus (an extension): the picture with a shallow depth of field
  normals : <out>/normals_npy/<name>_normals.npy  float32 [3,H,W] in [-1,1]
            <out>/normals_vis/<name>_normals.png   (n + 1) * 127.5
  iid     : <out>/iid_{appearance|lighting}_npy/<name>_<target>.npy  float32 [H,W,3] in [0,1]
            <out>/iid_{appearance|lighting}_vis/<name>_<target>.png  (script/iid/run.py:160-166, :260-270;
            the folder flavour is picked from the checkpoint name like the reference does)

Differences: the engine only runs on an MI355X (there is no CPU / MPS path: ``--apple_silicon`` is
accepted and refused); ``--half_precision`` / ``--fp16`` selects the ``fp16`` weight variant of the checkpoint AND the
fp16-operand build of the engine (fp32 accumulation), like the reference; without it the engine computes on bf16 operands.
"""
import argparse
import logging
import math
import os
from glob import glob

import numpy as np
from PIL import Image

EXTENSION_LIST = (".jpg", ".jpeg", ".png")
_DEFAULT_CKPT = {"depth": "prs-eth/marigold-depth-v1-1", "normals": "prs-eth/marigold-normals-v1-1",
                 "iid": "prs-eth/marigold-iid-appearance-v1-1"}
_TITLE = {"depth": "Marigold : Monocular Depth Estimation : Multi-image Inference",
          "normals": "Marigold : Surface Normals Estimation : Multi-image Inference",
          "iid": "Marigold : Intrinsic Image Decomposition : Multi-image Inference"}


def build_parser(kind: str) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=_TITLE[kind])
    p.add_argument("--checkpoint", type=str, default=_DEFAULT_CKPT[kind], help="Checkpoint path or hub name.")
    p.add_argument("--input_rgb_dir", type=str, required=True, help="Path to the input image folder.")
    p.add_argument("--output_dir", type=str, required=True, help="Output directory.")
    p.add_argument("--denoise_steps", type=int, default=None,
                   help="Diffusion denoising steps; `None` reads the default from the checkpoint.")
    p.add_argument("--processing_res", type=int, default=None,
                   help="Resolution the input is resized to before estimation; 0 = native, None = checkpoint default.")
    p.add_argument("--ensemble_size", type=int, default=1, help="Number of predictions to be ensembled.")
    p.add_argument("--half_precision", "--fp16", action="store_true",
                   help="Load the 16-bit weight variant of the checkpoint.")
    p.add_argument("--tiny_vae", type=str, default=None, metavar="DIR",
                   help="Folder of a diffusers AutoencoderTiny (e.g. a local copy of madebyollin/taesd): the pipeline encodes and decodes "
                        "with it in place of the checkpoint's VAE.")
    p.add_argument("--output_processing_res", action="store_true",
                   help="Output at the processing resolution instead of resizing back to the input resolution.")
    p.add_argument("--resample_method", choices=["bilinear", "bicubic", "nearest"], default="bilinear")
    if kind == "depth":
        p.add_argument("--color_map", type=str, default="Spectral", help="Colormap of the depth visualisation.")
    p.add_argument("--seed", type=int, default=None, help="Reproducibility seed; None = randomised inference.")
    p.add_argument("--batch_size", type=int, default=0, help="Inference batch size; 0 = automatic.")
    p.add_argument("--apple_silicon", action="store_true", help="(reference flag; not available on this engine)")
    p.add_argument("--maps_in_flight", type=int, default=0,
                   help="Images on the GPU at a time (independent maps on concurrent HIP streams; results do not depend on it); "
                        "0 = the engine's default (maps_in_flight_for: 3 lanes while a program holds 8 members or fewer on this GPU, else 2).")
    p.add_argument("--images_per_program", type=int, default=1,
                   help="Consecutive images of one processed size that share one denoising program (their members batched); "
                        "1 = one image per program.")
    p.add_argument("--sequence", action="store_true",
                   help="The sorted input files are consecutive frames of one sequence: every frame starts from the denoised latent of the "
                        "frame before (map_video). With --seed s, frame k draws its noise from the engine's own generator seeded s + k, "
                        "which a C host reproduces (mg_model_predict_next).")
    p.add_argument("--carry_strength", type=float, default=0.1,
                   help="--sequence: the weight of the previous frame's latent in a frame's initial latents; the noise gets 1 minus it.")
    if kind == "depth":   # (the other kinds have no affine ambiguity: there the flags are unknown arguments)
        p.add_argument("--sequence_align", action="store_true",
                       help="--sequence: fit every frame's depth map, scale and shift, robustly to the aligned map of the frame before "
                            "(or to the first frame's) on the GPU, so that the range stops changing from frame to frame "
                            "(map_video(align=...)).")
        p.add_argument("--align_delta", type=float, default=0.05,
                       help="--sequence_align: the residual, in depth units, at which a pixel's weight in the fit has fallen to a half.")
        p.add_argument("--align_iters", type=int, default=4, help="--sequence_align: reweighted solves per frame, 0 (plain least squares) to 32.")
        p.add_argument("--align_reference", choices=["previous", "first"], default="previous",
                       help="--sequence_align: what a frame is fitted to.")
    if kind == "depth":   # (depth to 3D, marigold_amd/points.py; the other kinds predict no depth: there the flags are unknown arguments)
        p.add_argument("--save_points", action="store_true",
                       help="Also write <output_dir>/depth_points/<name>_points.ply: the depth map as a point cloud in the camera's frame "
                            "(x right, y down, z forward) with the picture's colours, a binary PLY that 3D viewers open. Needs --fov_deg or "
                            "--focal_px.")
        p.add_argument("--fov_deg", type=float, default=None,
                       help="--save_points: the horizontal field of view of the input picture in degrees (square pixels, the principal "
                            "point at the centre).")
        p.add_argument("--focal_px", type=float, default=None,
                       help="--save_points: the focal length in pixels of the input picture, in place of --fov_deg.")
        p.add_argument("--points_near", type=float, default=1.0,
                       help="--save_points: the distance given to depth 0. The model's depth is affine-invariant, so near and far are the "
                            "user's choice; the defaults 1 and 10 are arbitrary.")
        p.add_argument("--points_far", type=float, default=10.0, help="--save_points: the distance given to depth 1 (z = near + d * (far - near)).")
        p.add_argument("--points_edge_rel", type=float, default=0.05,
                       help="--save_points: drop a pixel when a neighbour's distance differs by more than this fraction of the nearer one "
                            "(the flying pixels of a depth edge); 0 keeps them.")
        p.add_argument("--points_normals", action="store_true", help="--save_points: add the surface normal of every point to the records.")
        p.add_argument("--save_mesh", action="store_true",
                       help="Also write <output_dir>/depth_mesh/<name>_mesh.ply: the depth map as a triangle mesh in the camera's frame with "
                            "the picture's colours at its vertices, a binary PLY that 3D viewers open (marigold_amd/mesh.py). The camera, the "
                            "range, the edge rule and the normals are --save_points': --fov_deg or --focal_px, --points_near, --points_far, "
                            "--points_edge_rel (here: no triangle spans two distances that differ by more), --points_normals. May be given "
                            "with or without --save_points.")
        p.add_argument("--save_stereo", action="store_true",
                       help="Also write <output_dir>/depth_stereo/<name>_stereo.png: the picture seen by a left and a right eye, left "
                            "beside right at the map's size, rendered on the device from the triangles of --save_mesh "
                            "(marigold_amd/view.py). The camera, the range and the edge rule are --save_points': --fov_deg or --focal_px, "
                            "--points_near, --points_far, --points_edge_rel.")
        p.add_argument("--stereo_baseline", type=float, default=0.065,
                       help="--save_stereo: the distance between the two eyes, in the units of --points_near / --points_far. The default "
                            "rests on nothing measured: the distances themselves are the caller's choice.")
        p.add_argument("--stereo_fill", type=int, default=8,
                       help="--save_stereo: fill a pixel no triangle covers from the farther of the nearest covered pixels of its row, "
                            "within this many pixels (0 to 64; 0: leave the holes black). The default rests on nothing measured.")
        p.add_argument("--save_refocus", action="store_true",
                       help="Also write <output_dir>/depth_refocus/<name>_refocus.png: the picture at the map's size with a shallow depth "
                            "of field, every pixel blurred on the device by the circle of confusion of a thin lens focused at one distance "
                            "(marigold_amd/focus.py). The camera and the range are --save_points': --fov_deg or --focal_px, --points_near, "
                            "--points_far.")
        p.add_argument("--refocus_at", type=str, default="0.5,0.5",
                       help="--save_refocus: focus on the distance of this pixel, given as Y,X in fractions of the height and the width "
                            "(0,0: the top left corner; the default is the centre).")
        p.add_argument("--refocus_distance", type=float, default=None,
                       help="--save_refocus: focus at this distance, in the units of --points_near / --points_far, in place of --refocus_at.")
        p.add_argument("--refocus_aperture", type=float, default=0.1,
                       help="--save_refocus: the diameter of the lens, in the units of --points_near / --points_far; the blur radius in "
                            "pixels is half the focal length in pixels times this times |1 / z - 1 / focus|. No measurement stands behind "
                            "the default: the distances themselves are the caller's choice.")
        p.add_argument("--refocus_max_radius", type=int, default=16,
                       help="--save_refocus: the largest blur radius in pixels (0 to 32); larger ones are capped. No measurement stands "
                            "behind the default.")
    p.add_argument("--guided_upsample", action="store_true",
                   help="Enlarge the prediction to the input size with edge-guided (joint bilateral) upsampling in place of the plain "
                        "resampling: the input picture decides which low-resolution neighbours a pixel borrows from, so edges stay sharp.")
    p.add_argument("--guided_sigma", type=float, default=0.1,
                   help="--guided_upsample: the colour distance, on the 0 .. 1 scale, at which a neighbour stops counting.")
    p.add_argument("--guided_radius", type=int, default=2, help="--guided_upsample: the reach in low-resolution pixels, 1 to 4.")
    if kind != "iid":
        p.add_argument("--tile_size", type=int, default=0,
                       help="Predict every picture from overlapping square tiles of this size (a multiple of 8; 768 is the training size), "
                            "stitched on the GPU against a prediction of the whole picture at --processing_res (predict_tiled): for pictures "
                            "far larger than the processing resolution. 0 = no tiles. With --seed s the guide draws its noise from the "
                            "engine's own generator seeded s and tile i from s + 1 + i.")
        p.add_argument("--tile_overlap", type=int, default=0,
                       help="--tile_size: the minimum overlap of neighbouring tiles (a multiple of 8, at most half a tile); 0 = a quarter of the tile.")
        p.add_argument("--tiled_res", type=int, default=0,
                       help="--tile_size: the picture is first resized so that its longer edge has this length; 0 = tiles at the input resolution.")
    return p


def check_tile_args(args):
    """The tile flags against the rest of the command line, before anything is loaded."""
    if not getattr(args, "tile_size", 0):
        if getattr(args, "tile_overlap", 0) or getattr(args, "tiled_res", 0):
            raise ValueError("--tile_overlap and --tiled_res need --tile_size")
        return
    if args.sequence:
        raise ValueError("--tile_size cannot be combined with --sequence: a sequence carries one latent per frame, tiles have many")
    if args.images_per_program > 1:
        raise ValueError("--tile_size runs its tiles as the images of a program: --images_per_program must be 1")
    if args.tile_size < 16 or args.tile_size % 8 or args.tile_overlap < 0 or args.tile_overlap % 8 or 2 * args.tile_overlap > args.tile_size \
            or args.tiled_res < 0:
        raise ValueError(f"--tile_size {args.tile_size} / --tile_overlap {args.tile_overlap} / --tiled_res {args.tiled_res}: sizes are "
                         "multiples of 8, the tile 16 at least, the overlap at most half a tile")


def guided_upsample_arg(args):
    """The guided flags against the rest of the command line, before anything is loaded -> the pipelines' ``guided_upsample`` keyword,
    or None without ``--guided_upsample`` (the keyword is then not passed at all)."""
    if not args.guided_upsample:
        return None
    if args.output_processing_res:
        raise ValueError("--guided_upsample enlarges to the input size: it cannot be combined with --output_processing_res")
    if getattr(args, "tile_size", 0):
        raise ValueError("--guided_upsample cannot be combined with --tile_size")
    from .guided import settings
    radius, sigma = settings(dict(radius=args.guided_radius, sigma=args.guided_sigma))
    return dict(radius=radius, sigma=sigma)


def sequence_align_arg(parser, args):
    """The alignment flags against the rest of the command line, before anything is loaded -> ``map_video``'s ``align`` keyword, or None
    without ``--sequence_align`` (the keyword is then not passed at all).  What does not fit is an argparse error."""
    if not getattr(args, "sequence_align", False):
        return None
    if not args.sequence:
        parser.error("--sequence_align aligns consecutive frames: it needs --sequence")
    from .align import DepthAlignState
    try:
        DepthAlignState(iters=args.align_iters, delta=args.align_delta, reference=args.align_reference)
    except ValueError as e:
        parser.error(str(e))
    return dict(iters=args.align_iters, delta=args.align_delta, reference=args.align_reference)


def save_points_arg(parser, args, flag="--save_points"):
    """The point-cloud flags against the rest of the command line, before anything is loaded -> None without ``flag`` (``--save_points``,
    or ``--save_mesh``, which takes the same settings), else the settings ``save_points`` / ``save_mesh`` take.  What does not fit is an
    argparse error; the combination with ``--tile_size`` is refused like the other combinations with it."""
    if not getattr(args, flag[2:], False):
        return None
    if getattr(args, "tile_size", 0):
        raise ValueError(f"{flag} cannot be combined with --tile_size")
    if (args.fov_deg is None) == (args.focal_px is None):
        parser.error(f"{flag} needs the camera: exactly one of --fov_deg and --focal_px")
    if args.fov_deg is not None and not 0.0 < args.fov_deg < 180.0:
        parser.error(f"--fov_deg must lie inside (0, 180) (got {args.fov_deg})")
    if args.focal_px is not None and not (math.isfinite(args.focal_px) and args.focal_px > 0.0):
        parser.error(f"--focal_px must be finite and > 0 (got {args.focal_px})")
    if not (math.isfinite(args.points_near) and math.isfinite(args.points_far) and 0.0 <= args.points_near < args.points_far):
        parser.error(f"--points_near / --points_far must be finite with 0 <= near < far (got {args.points_near}, {args.points_far})")
    if not (math.isfinite(args.points_edge_rel) and args.points_edge_rel >= 0.0):
        parser.error(f"--points_edge_rel must be finite and >= 0 (got {args.points_edge_rel})")
    return dict(fov_deg=args.fov_deg, focal_px=args.focal_px, near=args.points_near, far=args.points_far, edge_rel=args.points_edge_rel,
                normals=args.points_normals)


def _map_camera_colours(rgb_path, out, cfg, device):
    """What ``save_points`` and ``save_mesh`` hand to the device call -> (depth on the device, K, the picture's planes at the map's size).
    The camera is given for the input picture and rescaled to the map's size where that differs (--output_processing_res); the colours
    are the picture's own, resampled to the map's size."""
    import torch
    from . import points as P
    from .util.image_util import InterpolationMode, resize
    depth = torch.from_numpy(np.ascontiguousarray(out.depth_np, dtype=np.float32)).to(device)
    h, w = depth.shape
    picture = torch.from_numpy(np.array(Image.open(rgb_path).convert("RGB"))).to(device)
    H, W = picture.shape[:2]
    if cfg["focal_px"] is not None:
        K = P.Intrinsics(cfg["focal_px"], cfg["focal_px"], (W - 1) / 2.0, (H - 1) / 2.0)
    else:
        K = P.intrinsics_from_fov(H, W, cfg["fov_deg"])
    planes = picture.permute(2, 0, 1)[None]
    if (H, W) != (h, w):
        K = P.scale_intrinsics(K, (H, W), (h, w))
        planes = resize(planes, (h, w), InterpolationMode.BILINEAR, antialias=True)
    return depth, K, planes[0].contiguous()


def save_points(folder, rgb_path, out, cfg, device):
    """``--save_points``: one picture's depth map as ``<folder>/<name>_points.ply`` -> the path.  z = near + depth * (far - near) goes in
    as ``coef``.  One read-back: the cloud's."""
    from . import points as P
    depth, K, planes = _map_camera_colours(rgb_path, out, cfg, device)
    cloud = P.depth_to_points(depth, K, colors=planes, coef=(cfg["far"] - cfg["near"], cfg["near"]), edge_rel=cfg["edge_rel"],
                              normals=cfg["normals"], frame="camera")
    path = os.path.join(folder, os.path.splitext(os.path.basename(rgb_path))[0] + "_points.ply")
    _save(path, cloud.write_ply)
    return path


def save_mesh(folder, rgb_path, out, cfg, device):
    """``--save_mesh``: one picture's depth map as ``<folder>/<name>_mesh.ply`` -> the path; the camera, the colours and ``coef`` as in
    ``save_points``.  One read-back: the mesh's."""
    from . import mesh as M
    depth, K, planes = _map_camera_colours(rgb_path, out, cfg, device)
    mesh = M.depth_to_mesh(depth, K, colors=planes, coef=(cfg["far"] - cfg["near"], cfg["near"]), edge_rel=cfg["edge_rel"],
                           normals=cfg["normals"], frame="camera")
    path = os.path.join(folder, os.path.splitext(os.path.basename(rgb_path))[0] + "_mesh.ply")
    _save(path, mesh.write_ply)
    return path


def save_stereo_arg(parser, args):
    """``--save_stereo`` against the rest of the command line -> None without it, else the settings ``save_stereo`` takes: those of
    ``--save_points`` with the baseline and the fill radius."""
    cfg = save_points_arg(parser, args, "--save_stereo")
    if cfg is None:
        return None
    if not math.isfinite(args.stereo_baseline):
        parser.error(f"--stereo_baseline must be finite (got {args.stereo_baseline})")
    if not 0 <= args.stereo_fill <= 64:
        parser.error(f"--stereo_fill must lie in 0 .. 64 (got {args.stereo_fill})")
    return dict(cfg, baseline=args.stereo_baseline, fill=args.stereo_fill)


def save_stereo(folder, rgb_path, out, cfg, device):
    """``--save_stereo``: one picture's stereo pair as ``<folder>/<name>_stereo.png``, left beside right -> the path; the camera, the
    colours and ``coef`` as in ``save_points``.  One read-back per eye: its picture."""
    from . import view as V
    depth, K, planes = _map_camera_colours(rgb_path, out, cfg, device)
    pair = V.stereo_pair(depth, K, planes, cfg["baseline"], coef=(cfg["far"] - cfg["near"], cfg["near"]), edge_rel=cfg["edge_rel"],
                         fill_radius=cfg["fill"])
    both = np.concatenate([eye.to_host().rgb for eye in pair], axis=1)
    path = os.path.join(folder, os.path.splitext(os.path.basename(rgb_path))[0] + "_stereo.png")
    _save(path, lambda tmp: Image.fromarray(both).save(tmp, format="PNG"))
    return path


def save_refocus_arg(parser, args):
    """``--save_refocus`` against the rest of the command line -> None without it, else the settings ``save_refocus`` takes: those of
    ``--save_points`` with the focus - ``at``, fractions (y, x), or ``distance`` - the aperture and the largest radius."""
    cfg = save_points_arg(parser, args, "--save_refocus")
    if cfg is None:
        return None
    try:
        fy, fx = (float(v) for v in args.refocus_at.split(","))
    except ValueError:
        fy = fx = math.nan
    if not (0.0 <= fy <= 1.0 and 0.0 <= fx <= 1.0):
        parser.error(f"--refocus_at must be Y,X, two fractions inside [0, 1] (got {args.refocus_at})")
    if args.refocus_distance is not None and not (math.isfinite(args.refocus_distance) and args.refocus_distance > 0.0):
        parser.error(f"--refocus_distance must be finite and > 0 (got {args.refocus_distance})")
    if not (math.isfinite(args.refocus_aperture) and args.refocus_aperture >= 0.0):
        parser.error(f"--refocus_aperture must be finite and >= 0 (got {args.refocus_aperture})")
    if not 0 <= args.refocus_max_radius <= 32:
        parser.error(f"--refocus_max_radius must lie in 0 .. 32 (got {args.refocus_max_radius})")
    return dict(cfg, at=(fy, fx), distance=args.refocus_distance, aperture=args.refocus_aperture, max_radius=args.refocus_max_radius)


def save_refocus(folder, rgb_path, out, cfg, device):
    """``--save_refocus``: one picture refocused as ``<folder>/<name>_refocus.png`` at the map's size -> the path; the camera, the
    colours and ``coef`` as in ``save_points``.  The focus pixel is the fraction of the map's size, rounded down and kept inside the
    map; its distance is read on the device.  One read-back: the picture."""
    from . import focus as F
    depth, K, planes = _map_camera_colours(rgb_path, out, cfg, device)
    h, w = depth.shape
    if cfg["distance"] is not None:
        where = dict(focus=cfg["distance"])
    else:
        where = dict(focus_at=(min(int(cfg["at"][0] * h), h - 1), min(int(cfg["at"][1] * w), w - 1)))
    shot = F.refocus(depth, planes, K=K, aperture=cfg["aperture"], max_radius=cfg["max_radius"], coef=(cfg["far"] - cfg["near"], cfg["near"]),
                     **where)
    picture = shot.to_host().rgb
    path = os.path.join(folder, os.path.splitext(os.path.basename(rgb_path))[0] + "_refocus.png")
    _save(path, lambda tmp: Image.fromarray(picture).save(tmp, format="PNG"))
    return path


def list_images(folder):
    files = sorted(f for f in glob(os.path.join(folder, "*")) if os.path.splitext(f)[1].lower() in EXTENSION_LIST)
    return files


def output_dirs(kind, output_dir, checkpoint=""):
    if kind == "iid":
        flavour = "appearance" if "appearance" in checkpoint else "lighting"
        dirs = {"iid_vis": os.path.join(output_dir, f"iid_{flavour}_vis"),
                "iid_npy": os.path.join(output_dir, f"iid_{flavour}_npy")}
    else:
        sub = ("depth_colored", "depth_bw", "depth_npy") if kind == "depth" else ("normals_vis", "normals_npy")
        dirs = {s: os.path.join(output_dir, s) for s in sub}
    for d in (output_dir, *dirs.values()):
        os.makedirs(d, exist_ok=True)
    return dirs


def _save(path, writer):
    if os.path.exists(path):
        logging.warning(f"Existing file: '{path}' will be overwritten")
    writer(path)


def save_prediction(kind, dirs, rgb_path, out):
    """Write one prediction in the reference's formats; returns the written paths."""
    base = os.path.splitext(os.path.basename(rgb_path))[0]
    written = []
    if kind == "depth":
        name = base + "_depth"
        depth = out.depth_np
        p = os.path.join(dirs["depth_npy"], f"{name}.npy")
        _save(p, lambda q: np.save(q, depth))
        written.append(p)
        p = os.path.join(dirs["depth_bw"], f"{name}.png")
        _save(p, lambda q: Image.fromarray((depth * 65535.0).astype(np.uint16)).save(q, mode="I;16"))
        written.append(p)
        if out.depth_colored is not None:
            p = os.path.join(dirs["depth_colored"], f"{name}_colored.png")
            _save(p, out.depth_colored.save)
            written.append(p)
    elif kind == "iid":
        for entry in out:
            arr = np.moveaxis(entry.array, 0, -1)   # chw2hwc
            p = os.path.join(dirs["iid_npy"], f"{base}_{entry.name}.npy")
            _save(p, lambda q: np.save(q, arr))
            written.append(p)
            p = os.path.join(dirs["iid_vis"], f"{base}_{entry.name}.png")
            _save(p, entry.image.save)
            written.append(p)
    else:
        name = base + "_normals"
        p = os.path.join(dirs["normals_npy"], f"{name}.npy")
        _save(p, lambda q: np.save(q, out.normals_np))
        written.append(p)
        p = os.path.join(dirs["normals_vis"], f"{name}.png")
        _save(p, out.normals_img.save)
        written.append(p)
    return written


def apply_tiny_vae(pipeline, folder, half_precision=False):
    """``--tiny_vae DIR``: load the tiny autoencoder of ``folder`` with the pipeline's operand type and swap it in."""
    import torch
    from .checkpoint import load_tiny_vae
    pipeline.set_vae(load_tiny_vae(folder, variant="fp16" if half_precision else None,
                                   torch_dtype=torch.float16 if half_precision else torch.float32))
    logging.info(f"VAE: the tiny autoencoder of `{folder}`")
    return pipeline


def main(kind: str, argv=None, pipeline=None) -> int:
    """``pipeline`` lets tests inject a ready pipeline object; otherwise the checkpoint is loaded."""
    import torch
    logging.basicConfig(level=logging.INFO)
    parser = build_parser(kind)
    args = parser.parse_args(argv)
    check_tile_args(args)
    guided = guided_upsample_arg(args)
    align = sequence_align_arg(parser, args)
    points = save_points_arg(parser, args)
    mesh = save_points_arg(parser, args, "--save_mesh")
    stereo = save_stereo_arg(parser, args)
    refocus = save_refocus_arg(parser, args)
    if args.ensemble_size > 15:
        logging.warning("Running with large ensemble size will be slow.")
    match_input_res = not args.output_processing_res
    if 0 == args.processing_res and match_input_res is False:
        logging.warning("Processing at native resolution without resizing output might NOT lead to exactly the "
                        "same resolution, due to the padding and pooling properties of conv layers.")
    if args.apple_silicon:
        raise RuntimeError("--apple_silicon: this engine runs on an AMD MI355X only")
    dirs = output_dirs(kind, args.output_dir, args.checkpoint)
    logging.info(f"output dir = {args.output_dir}")
    files = list_images(args.input_rgb_dir)
    if not files:
        logging.error(f"No image found in '{args.input_rgb_dir}'")
        return 1
    logging.info(f"Found {len(files)} images")
    if points is not None:
        points_dir = os.path.join(args.output_dir, "depth_points")
        os.makedirs(points_dir, exist_ok=True)
    if mesh is not None:
        mesh_dir = os.path.join(args.output_dir, "depth_mesh")
        os.makedirs(mesh_dir, exist_ok=True)
    if stereo is not None:
        stereo_dir = os.path.join(args.output_dir, "depth_stereo")
        os.makedirs(stereo_dir, exist_ok=True)
    if refocus is not None:
        refocus_dir = os.path.join(args.output_dir, "depth_refocus")
        os.makedirs(refocus_dir, exist_ok=True)
    if pipeline is None:
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible: the Marigold HIP engine has no CPU fallback")
        import marigold_amd as M
        cls = {"depth": M.MarigoldDepthPipeline, "normals": M.MarigoldNormalsPipeline,
               "iid": M.MarigoldIIDPipeline}[kind]
        pipeline = cls.from_pretrained(args.checkpoint, variant="fp16" if args.half_precision else None,
                                       torch_dtype=torch.float16 if args.half_precision else torch.float32)
        pipeline.enable_xformers_memory_efficient_attention()   # no-op: attention is always the fused kernel
        pipeline = pipeline.to("cuda")
    if args.tiny_vae:
        apply_tiny_vae(pipeline, args.tiny_vae, args.half_precision)
    if kind == "depth":
        logging.info(f"Loaded depth pipeline: scale_invariant={pipeline.scale_invariant}, "
                     f"shift_invariant={pipeline.shift_invariant}")
    elif kind == "iid":
        logging.info(f"Loaded IID pipeline with predicted target names: {pipeline.target_names}")
    else:
        logging.info("Loaded normals pipeline")
    logging.info(f"Inference settings: checkpoint = `{args.checkpoint}`, with denoise_steps = "
                 f"{args.denoise_steps or pipeline.default_denoising_steps}, ensemble_size = {args.ensemble_size}, "
                 f"processing resolution = {args.processing_res or pipeline.default_processing_resolution}, "
                 f"seed = {args.seed}" + (f"; color_map = {args.color_map}." if kind == "depth" else ""))
    device = getattr(pipeline, "device", "cpu")
    kw = dict(denoising_steps=args.denoise_steps, ensemble_size=args.ensemble_size,
              processing_res=args.processing_res, match_input_res=match_input_res,
              batch_size=args.batch_size, show_progress_bar=True, resample_method=args.resample_method)
    if kind == "depth":
        kw["color_map"] = args.color_map
    if guided is not None:
        kw["guided_upsample"] = guided

    def generator_of(_path):   # a fresh generator per image, like the reference's loop (script/depth/run.py:240-244)
        if args.seed is None:
            return None
        g = torch.Generator(device=device)
        g.manual_seed(args.seed)
        return g

    def save(rgb_path, out):
        save_prediction(kind, dirs, rgb_path, out)
        if points is not None:
            save_points(points_dir, rgb_path, out, points, device)
        if mesh is not None:
            save_mesh(mesh_dir, rgb_path, out, mesh, device)
        if stereo is not None:
            save_stereo(stereo_dir, rgb_path, out, stereo, device)
        if refocus is not None:
            save_refocus(refocus_dir, rgb_path, out, refocus, device)

    if args.images_per_program < 1:
        raise ValueError(f"--images_per_program must be >= 1 (got {args.images_per_program})")
    if args.sequence:
        # consecutive frames: map_video in place of map_images; frame k's noise is NativeNoise(seed + k)
        if args.images_per_program > 1:
            raise ValueError("--sequence runs one frame per program: --images_per_program must be 1")
        if not hasattr(pipeline, "map_video"):
            raise RuntimeError("--sequence needs a pipeline with map_video")
        from .noise import NativeNoise
        seeds = (None if args.seed is None else NativeNoise(args.seed + k) for k in range(len(files)))
        video_kw = dict(kw) if align is None else dict(kw, align=align)
        outs = pipeline.map_video((Image.open(f) for f in files), strength=args.carry_strength, in_flight=args.maps_in_flight or None,
                                  generators=seeds, **video_kw)
        for rgb_path, out in zip(files, outs):
            save(rgb_path, out)
    elif getattr(args, "tile_size", 0):
        # large pictures: each from overlapping tiles, stitched on the device; --processing_res is the guide's resolution
        if not hasattr(pipeline, "predict_tiled"):
            raise RuntimeError("--tile_size needs a pipeline with predict_tiled")
        from .noise import NativeNoise
        tile_kw = {k: v for k, v in kw.items() if k != "processing_res"}
        overlap = args.tile_overlap or max(8, args.tile_size // 4 // 8 * 8)
        for rgb_path in files:
            out = pipeline.predict_tiled(Image.open(rgb_path), tile_size=args.tile_size, tile_overlap=overlap, tiled_res=args.tiled_res,
                                         guide_res=args.processing_res, in_flight=args.maps_in_flight or None,
                                         generator=None if args.seed is None else NativeNoise(args.seed), **tile_kw)
            if getattr(out, "degenerate_tiles", None):
                logging.warning(f"{rgb_path}: {out.degenerate_tiles} tile(s) could not be fitted to the guide and carry its mean")
            save(rgb_path, out)
    elif hasattr(pipeline, "map_images"):
        # the engine's multi-image form: up to --maps_in_flight images on the GPU at a time, outputs in input order
        if args.images_per_program > 1:
            kw["images_per_program"] = args.images_per_program
        outs = pipeline.map_images((Image.open(f) for f in files), in_flight=args.maps_in_flight or None,
                                   generators=(generator_of(f) for f in files), **kw)
        for rgb_path, out in zip(files, outs):
            save(rgb_path, out)
    else:   # an object with the reference pipeline's call surface only
        for rgb_path in files:
            out = pipeline(Image.open(rgb_path), generator=generator_of(rgb_path), **kw)
            save(rgb_path, out)
    return 0
