"""Command-line entry points with the reference scripts' arguments.

    python -m vcamd.cli encode_B --ref_1 frames/ref_1.png --ref_2 frames/ref_2.png --current frames/current.png --bin bits_B.bin --l 1626
    python -m vcamd.cli decode_B --ref_1 frames/ref_1.png --ref_2 frames/ref_2.png --bin bits_B.bin [--out decoded.png]
    python -m vcamd.cli test --test_path /datasets/UVG/full_test/ --b_pretrained ../new_compression_1626.pth --lmbda 1626
    python -m vcamd.cli encode_seq --frames DIR --out FILE --level S [--intra_size 16] [--weights B.pth --i_weights I.pth | --seeded N]
    python -m vcamd.cli decode_seq --bin FILE --out DIR [--weights B.pth --i_weights I.pth | --seeded N]
    python -m vcamd.cli encode_seq_lhbdc --frames DIR --out FILE [--l 1626] [--i_qual 7] [--weights B.pth --i_weights I.pth | --seeded N] [--no_hash]
    python -m vcamd.cli decode_seq_lhbdc --bin FILE --out DIR [--l 1626] [--i_qual 7] [--weights B.pth --i_weights I.pth | --seeded N] [--no_verify]

``encode_B`` / ``decode_B`` mirror LHBDC/encode_B.py:21-28,108-126 and LHBDC/decode_B.py:23-28,88-124 (same argument
names and defaults, same ``bits_B.bin`` container, ``decoded.png`` written beside the bitstream); ``test`` mirrors the
argument parser and the loop of LHBDC/test/testing.py:35-59,89-196 on top of ``vcamd.data.SequenceReader``; ``test --msssim`` adds
an MS-SSIM column (pytorch-msssim ``ms_ssim`` defaults on the same uint8 crops, computed on the device) to every line it prints.

``encode_seq`` / ``decode_seq`` are the ICIP2024 models as a whole-sequence codec (vcamd.sequence): the PNGs of a folder, in name
order, into one ``VCSQ`` file (device-coded ELIC I-frames and FlowGuidedB B-frames) and back into ``im00001.png`` ... of the unpadded
picture, from the file and the two checkpoints alone.

``encode_seq_lhbdc`` / ``decode_seq_lhbdc`` do the same with the LHBDC model between mbt2018_mean I-frames (vcamd.sequence.
LhbdcSequenceCodec): one ``VCLS`` file that carries a hash of every decoded picture unless ``--no_hash`` is given; the decoder recomputes
the hashes and fails on the first frame whose reconstruction is not the encoder's unless ``--no_verify`` is given.

Checkpoints: ``--weights`` (default ``pretrained_weights/compression_<l>.pth``, as the reference) is loaded with
``torch.load(...)["state_dict"]``.  The reference's checkpoints live on Google Drive; where none is present ``--seeded
SEED`` runs the same code on the deterministic synthetic checkpoint of ``vcamd.seeding`` (encoder and decoder must use
the same seed).  Everything runs on the HIP path: a CUDA device is required.
"""
import argparse
import os
import sys

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from vcamd import hip, lhbdc  # noqa: E402
from vcamd.data import SequenceReader, read_png, write_png  # noqa: E402

LAMBDAS = [228, 436, 845, 1626, 3141]


def _device():
    if not torch.cuda.is_available():
        raise hip.VcError("vcamd.cli runs on the HIP path only: no CUDA/ROCm device is visible (there is no CPU fallback)")
    return torch.device("cuda")


def load_b_model(l, weights=None, seeded=None, device=None):
    """encode_B.py:32-37: Model(), load_state_dict, update(force=True) on both codecs, eval()."""
    device = device or _device()
    model = lhbdc.Model()
    if seeded is not None:
        from vcamd.seeding import seeded_state_dict
        model.load_state_dict(seeded_state_dict(model.state_dict(), seed=int(seeded)))
    else:
        path = weights or f"pretrained_weights/compression_{l}.pth"
        if not os.path.exists(path):
            raise hip.VcError(f"checkpoint {path} not found (the reference's weights are a separate download); pass --weights PATH "
                              "or --seeded SEED for the synthetic checkpoint")
        model.load_state_dict(torch.load(path, map_location=lambda storage, loc: storage)["state_dict"])
    model.mv_compressor.update(force=True)
    model.residual_compressor.update(force=True)
    return model.to(device).float().eval()


def frame_from_file(path, device):
    """``process_frame(imageio.imread(path).astype(float))`` (encode_B.py:58-64,109-111) with the pixel work on the device:
    returns the padded fp32 NCHW tensor and the original (h, w)."""
    rgb = read_png(path)
    x = hip.frame_from_uint8(torch.from_numpy(rgb).to(device))
    return x, rgb.shape[:2]


def cmd_encode_B(args):
    dev = _device()
    model = load_b_model(args.l, args.weights, args.seeded, dev)
    with torch.no_grad():
        x_before, _ = frame_from_file(args.ref_1, dev)
        x_after, _ = frame_from_file(args.ref_2, dev)
        x_current, _ = frame_from_file(args.current, dev)
        mv_bits, res_bits = lhbdc.encode_B(model, x_after, x_current, x_before)
    blob = lhbdc.write_container(args.bin, args.l, mv_bits, res_bits)
    print(f"{args.bin}: {len(blob)} bytes ({8.0 * len(blob) / (x_current.shape[-1] * x_current.shape[-2]):.4f} bpp on the padded frame)")
    return blob


def cmd_decode_B(args):
    dev = _device()
    l, mv_bits_dec, res_bits_dec, shape_mv, shape_res = lhbdc.read_container(args.bin)
    model = load_b_model(int(l), args.weights, args.seeded, dev)
    with torch.no_grad():
        x_before, (h, w) = frame_from_file(args.ref_1, dev)
        x_after, _ = frame_from_file(args.ref_2, dev)
        decoded = lhbdc.decode_B(x_before, x_after, model, mv_bits_dec, res_bits_dec, shape_mv, shape_res)
        u8 = hip.frame_to_uint8(decoded[:1], h, w).cpu().numpy()
    write_png(args.out, u8)
    print(f"{args.out}: {w}x{h}")
    return u8


def cmd_test(args):
    """testing.py:65-196: every sequence under --test_path, GOP by GOP, I-frames through mbt2018_mean(--i_qual),
    B-frames through the model; prints the per-level and overall (PSNR, bpp) table (``--msssim``: with an MS-SSIM column)."""
    from vcamd import gop
    from vcamd.iframe import mbt2018_mean
    dev = _device()
    model = load_b_model(args.lmbda, args.b_pretrained, args.seeded, dev)
    i_model = mbt2018_mean(args.i_qual, "mse", pretrained=False)
    if args.seeded is not None or not args.i_pretrained:
        from vcamd.seeding import seeded_state_dict
        i_model.load_state_dict(seeded_state_dict(i_model.state_dict(), seed=4321, conv_gain=0.8))
    else:
        i_model.load_state_dict(torch.load(args.i_pretrained, map_location="cpu"))
    i_model.update(force=True)
    i_model = i_model.to(dev).float().eval()
    reader = SequenceReader(args.test_path, None, args.test_gop_size, args.test_skip_frames, args.test_numbers, dev, args.workers,
                            yuv_size=tuple(args.yuv_size) if args.yuv_size else None)
    table = gop.RdTable()

    def ms(v):
        return f"  MS-SSIM {v['msssim']:.4f}" if args.msssim else ""
    with torch.no_grad():
        for vi, name in enumerate(reader.video_names):
            avail = (len(reader.videos[vi]) + reader.skip_frames - 1) // reader.skip_frames
            reader.prefetch([k for k in reader.items if k[0] == vi])
            rows = gop.code_sequence_lhbdc(model, i_model, lambda idx, vi=vi: reader.load_frame(vi, idx), avail, reader.h, reader.w,
                                           video=vi, gop_size=args.test_gop_size, test_size=args.test_numbers, msssim=args.msssim)
            rows = gop.gather_records(rows, dev)                 # one D2H of the per-frame scalars, (video, frame) order
            for r in rows.tolist():
                table.update("I" if int(r[6]) == 1 else "B", r[1], int(r[2]), int(r[0]), r[3], r[4], r[5], r[7] if args.msssim else None)
            s = gop.summarize(rows)
            print(f"{name}: {s['frames']} frames  PSNR {s['psnr']:.3f} dB  {s['bpp']:.4f} bpp{ms(s)}", flush=True)
    summary = {"per_level": table.per_level(), "per_level_frame_type": table.per_level_frame_type(),
               "overall": table._group(lambda r: 0).get(0)}
    for level, v in summary["per_level"].items():
        print(f"level {level:2d}: {v['frames']:4d} frames  PSNR {v['psnr']:.3f} dB  {v['bpp']:.4f} bpp{ms(v)}")
    print(f"overall : {summary['overall']['frames']:4d} frames  PSNR {summary['overall']['psnr']:.3f} dB  {summary['overall']['bpp']:.4f} bpp{ms(summary['overall'])}")
    st = reader.stats
    print(f"ingest: {st['frames']} frames, decode {st['decode_s']:.2f} s (worker time), H2D {st['h2d_s']:.2f} s, consumer waited "
          f"{st['wait_s']:.2f} s")
    reader.close()
    return summary


def _seq_codec(args, dev):
    from vcamd import sequence
    model, intra = sequence.load_models(args.seeded, args.weights, args.i_weights, dev)
    return sequence.Icip2024SequenceCodec(model, intra, waves=args.waves, intra_quality=args.i_qual)


def _png_folder(folder, dev):
    """(names in coding = name order, h, w, load_frame(i) -> padded NCHW frame on ``dev``) of a folder of PNG frames"""
    names = sorted(n for n in os.listdir(folder) if n.lower().endswith(".png"))
    if not names:
        raise hip.VcError(f"{folder}: no PNG frames")
    first = read_png(os.path.join(folder, names[0]))
    h, w = first.shape[:2]

    def load_frame(i):
        rgb = first if i == 0 else read_png(os.path.join(folder, names[i]))
        if rgb.shape[:2] != (h, w):
            raise hip.VcError(f"{names[i]}: {rgb.shape[1]}x{rgb.shape[0]}, the sequence is {w}x{h}")
        return hip.frame_from_uint8(torch.from_numpy(rgb).to(dev))
    return names, h, w, load_frame


def cmd_encode_seq(args):
    dev = _device()
    names, h, w, load_frame = _png_folder(args.frames, dev)
    codec = _seq_codec(args, dev)
    with torch.no_grad():
        data, _ = codec.encode(load_frame, len(names), args.level, h, w, intra_size=args.intra_size)
    with open(args.out, "wb") as f:
        f.write(data)
    print(f"{args.out}: {len(names)} frames, {len(data)} bytes ({8.0 * len(data) / (len(names) * h * w):.4f} bpp)")
    return data


def cmd_decode_seq(args):
    from vcamd import containers, sequence
    dev = _device()
    with open(args.bin, "rb") as f:
        data = f.read()
    head = containers.unpack_sequence(data)
    codec = _seq_codec(args, dev)
    with torch.no_grad():
        frames = codec.decode(data)
    os.makedirs(args.out, exist_ok=True)
    for order in sorted(frames):
        write_png(os.path.join(args.out, f"im{order + 1:05d}.png"), sequence.crop_uint8(frames[order], head["height"], head["width"]))
    print(f"{args.out}: {len(frames)} frames of {head['width']}x{head['height']} from {len(data)} bytes")
    return frames


def _lhbdc_seq_codec(args, dev, **kw):
    from vcamd import sequence
    model, intra = sequence.load_lhbdc_models(args.seeded, args.weights, args.i_weights, args.i_qual, args.l, dev)
    return sequence.LhbdcSequenceCodec(model, intra, lmbda=args.l, waves=args.waves, intra_quality=args.i_qual, **kw)


def cmd_encode_seq_lhbdc(args):
    dev = _device()
    names, h, w, load_frame = _png_folder(args.frames, dev)
    codec = _lhbdc_seq_codec(args, dev, picture_hash=not args.no_hash)
    with torch.no_grad():
        data, _ = codec.encode(load_frame, len(names), h, w)
    with open(args.out, "wb") as f:
        f.write(data)
    print(f"{args.out}: {len(names)} frames, {len(data)} bytes ({8.0 * len(data) / (len(names) * h * w):.4f} bpp), "
          f"{'with' if codec.picture_hash else 'without'} picture hashes")
    return data


def cmd_decode_seq_lhbdc(args):
    from vcamd import containers, sequence
    dev = _device()
    with open(args.bin, "rb") as f:
        data = f.read()
    head = containers.unpack_lhbdc_sequence(data)
    codec = _lhbdc_seq_codec(args, dev)
    with torch.no_grad():
        frames = codec.decode(data, verify=not args.no_verify)
    os.makedirs(args.out, exist_ok=True)
    for order in sorted(frames):
        write_png(os.path.join(args.out, f"im{order + 1:05d}.png"), sequence.crop_uint8(frames[order], head["height"], head["width"]))
    print(f"{args.out}: {len(frames)} frames of {head['width']}x{head['height']} from {len(data)} bytes, picture hashes "
          f"{'verified' if codec.report['verified'] else 'not verified'}")
    return frames


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m vcamd.cli", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)

    def ckpt(p):
        p.add_argument("--weights", default=None, help="checkpoint with a 'state_dict' entry (default pretrained_weights/compression_<l>.pth)")
        p.add_argument("--seeded", type=int, default=None, help="use the synthetic checkpoint of vcamd.seeding with this seed instead")

    e = sub.add_parser("encode_B", formatter_class=argparse.ArgumentDefaultsHelpFormatter)      # encode_B.py:21-28
    e.add_argument("--ref_1", default="frames/ref_1.png")
    e.add_argument("--ref_2", default="frames/ref_2.png")
    e.add_argument("--current", default="frames/current.png")
    e.add_argument("--bin", default="bits_B.bin")
    e.add_argument("--l", type=int, default=1626, choices=LAMBDAS)
    ckpt(e)
    e.set_defaults(fn=cmd_encode_B)

    d = sub.add_parser("decode_B", formatter_class=argparse.ArgumentDefaultsHelpFormatter)      # decode_B.py:23-28
    d.add_argument("--ref_1", default="frames/ref_1.png")
    d.add_argument("--ref_2", default="frames/ref_2.png")
    d.add_argument("--bin", default="bits_B.bin")
    d.add_argument("--out", default="decoded.png")
    ckpt(d)
    d.set_defaults(fn=cmd_decode_B)

    t = sub.add_parser("test", formatter_class=argparse.ArgumentDefaultsHelpFormatter)          # test/testing.py:35-59
    t.add_argument("--project_name", type=str, default="LHBDC_test")
    t.add_argument("--model_name", type=str, default="Single_level_1626")
    t.add_argument("--test_path", type=str, default="/datasets/UVG/full_test/")
    t.add_argument("--test_gop_size", type=int, default=8)
    t.add_argument("--i_interval", type=int, default=8)
    t.add_argument("--test_skip_frames", type=int, default=1)
    t.add_argument("--test_numbers", type=int, default=None)
    t.add_argument("--device", type=str, default="cuda")
    t.add_argument("--workers", type=int, default=4)
    t.add_argument("--b_pretrained", type=str, default="../new_compression_1626.pth")
    t.add_argument("--i_pretrained", type=str, default=None, help="state dict of the mbt2018_mean I-frame codec (zoo weights are a download)")
    t.add_argument("--i_qual", type=int, default=7)
    t.add_argument("--lmbda", type=int, default=1626)
    t.add_argument("--yuv_size", type=int, nargs=2, default=None, metavar=("W", "H"), help="sequences are raw 8-bit 4:2:0 files of this size")
    t.add_argument("--seeded", type=int, default=None)
    t.add_argument("--msssim", action="store_true", help="also report MS-SSIM (pytorch-msssim ms_ssim defaults, data range 255) per sequence, level and overall")
    t.set_defaults(fn=cmd_test)

    def seq_ckpt(p):
        p.add_argument("--weights", default=None, help="FlowGuidedB checkpoint (a state dict, or one under 'state_dict')")
        p.add_argument("--i_weights", default=None, help="ELIC checkpoint of the I-frames")
        p.add_argument("--seeded", type=int, default=None, help="use the synthetic checkpoints of vcamd.seeding with this seed instead")
        p.add_argument("--i_qual", type=int, default=0, help="quality index of the I-frame checkpoint, carried in the file and checked by decode_seq")
        p.add_argument("--waves", type=int, default=4, help="sub-streams per payload of the device coder")

    es = sub.add_parser("encode_seq", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    es.add_argument("--frames", required=True, help="folder of PNG frames, coded in name order")
    es.add_argument("--out", required=True, help="the VCSQ file to write")
    es.add_argument("--level", type=float, required=True, help="quality level s of the B-frames")
    es.add_argument("--intra_size", type=int, default=16)
    seq_ckpt(es)
    es.set_defaults(fn=cmd_encode_seq)

    ds = sub.add_parser("decode_seq", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ds.add_argument("--bin", required=True, help="the VCSQ file")
    ds.add_argument("--out", required=True, help="folder for im00001.png ...")
    seq_ckpt(ds)
    ds.set_defaults(fn=cmd_decode_seq)

    def lhbdc_seq_ckpt(p):
        p.add_argument("--l", type=int, default=1626, choices=LAMBDAS)
        p.add_argument("--i_qual", type=int, default=7, choices=range(1, 9), help="mbt2018_mean quality of the I-frames, carried in the file")
        p.add_argument("--weights", default=None, help="LHBDC checkpoint with a 'state_dict' entry (default pretrained_weights/compression_<l>.pth)")
        p.add_argument("--i_weights", default=None, help="state dict of the mbt2018_mean I-frame codec")
        p.add_argument("--seeded", type=int, default=None, help="use the synthetic checkpoints of vcamd.seeding with this seed instead")
        p.add_argument("--waves", type=int, default=4, help="sub-streams per payload of the device coder")

    el = sub.add_parser("encode_seq_lhbdc", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    el.add_argument("--frames", required=True, help="folder of PNG frames, coded in name order")
    el.add_argument("--out", required=True, help="the VCLS file to write")
    el.add_argument("--no_hash", action="store_true", help="store no hash of the decoded pictures")
    lhbdc_seq_ckpt(el)
    el.set_defaults(fn=cmd_encode_seq_lhbdc)

    dl = sub.add_parser("decode_seq_lhbdc", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    dl.add_argument("--bin", required=True, help="the VCLS file")
    dl.add_argument("--out", required=True, help="folder for im00001.png ...")
    dl.add_argument("--no_verify", action="store_true", help="do not recompute the picture hashes of the file")
    lhbdc_seq_ckpt(dl)
    dl.set_defaults(fn=cmd_decode_seq_lhbdc)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    return args.fn(args)


if __name__ == "__main__":
    main()
