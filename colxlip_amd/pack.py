"""Write a packed image-text dataset: decode once, offline, so that training moves raw uint8 bytes and the device does the rest
(`data.PackedLoader`, `ops.image_transform`).

    python -m colxlip_amd.pack --csv captions.tsv --model ViT-B-32 --out DIR [--max-side 256]

A packed directory holds
    images.u8    concatenated HWC uint8 RGB images, each starting on a 64-byte boundary
    index.npy    int64 [n, 3]: byte offset, height, width
    tokens.npy   int32 [n, K, L]: K captions per image, tokenised to context length L
    meta.json    n, K, context_length, vocab_size, tokenizer
The CSV flags are the reference's (`--csv-img-key filepath --csv-caption-key title --csv-separator '\\t'`, reference
params.py:442-463); images are decoded with PIL and `.convert('RGB')` as the reference's datasets do (data.py:732).  K > 1 comes
from several caption columns (`--csv-caption-key a,b`) or from a `|||`-separated caption field; every row must give the same K.
`--max-side N` shrinks an image whose shortest side exceeds N to N (PIL bicubic, aspect kept) before it is stored, which keeps
stored images within the transform kernel's scale limit and the dataset small."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ALIGN = 64
CAPTION_SPLIT = "|||"
FILES = ("images.u8", "index.npy", "tokens.npy", "meta.json")


def _aligned(nbytes: int) -> int:
    return (nbytes + ALIGN - 1) // ALIGN * ALIGN


def decode_rgb(path, max_side=None) -> np.ndarray:
    """uint8 [h, w, 3] of an image file: PIL decode + convert('RGB'); shortest side shrunk to `max_side` when larger"""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        if max_side and min(im.size) > max_side:
            w, h = im.size
            s = max_side / min(w, h)
            im = im.resize((max(max_side, round(w * s)), max(max_side, round(h * s))), Image.BICUBIC)
        return np.asarray(im, dtype=np.uint8)


def write_packed(out_dir, images, captions, tokenizer, tokenizer_name="", context_length=None):
    """images: iterable of uint8 [h, w, 3] arrays; captions: list (one entry per image) of K strings each.  Returns meta."""
    os.makedirs(out_dir, exist_ok=True)
    ks = {len(c) for c in captions}
    if len(ks) != 1 or 0 in ks:
        raise ValueError(f"every image needs the same, non-zero number of captions (found {sorted(ks)})")
    K = ks.pop()
    index, pos = [], 0
    with open(os.path.join(out_dir, "images.u8"), "wb") as f:
        for arr in images:
            arr = np.ascontiguousarray(arr, dtype=np.uint8)
            if arr.ndim != 3 or arr.shape[2] != 3:
                raise ValueError(f"image {len(index)}: expected [h, w, 3] uint8, got {arr.shape}")
            f.write(arr.tobytes())
            index.append((pos, arr.shape[0], arr.shape[1]))
            end = pos + arr.size
            pos = _aligned(end)
            f.write(b"\0" * (pos - end))
    if len(index) != len(captions):
        raise ValueError(f"{len(index)} images but {len(captions)} caption rows")
    flat = [c for row in captions for c in row]
    toks = tokenizer(flat, context_length=context_length) if context_length else tokenizer(flat)
    toks = np.asarray(toks, dtype=np.int64)
    L = toks.shape[1]
    vocab = int(getattr(tokenizer, "vocab_size", 0)) or int(toks.max()) + 1
    np.save(os.path.join(out_dir, "index.npy"), np.asarray(index, dtype=np.int64).reshape(-1, 3))
    np.save(os.path.join(out_dir, "tokens.npy"), toks.astype(np.int32).reshape(len(index), K, L))
    meta = {"n": len(index), "K": K, "context_length": L, "vocab_size": vocab, "tokenizer": tokenizer_name}
    with open(os.path.join(out_dir, "meta.json"), "w") as f:
        json.dump(meta, f)
    return meta


def read_csv(path, img_key="filepath", caption_key="title", separator="\t"):
    """([image path], [[caption] * K]) of a captions table; relative image paths are taken relative to the table's directory"""
    keys = [k for k in caption_key.split(",") if k]
    base = os.path.dirname(os.path.abspath(path))
    paths, captions = [], []
    with open(path, newline="") as f:
        for row in csv.DictReader(f, delimiter=separator):
            caps = []
            for k in keys:
                caps.extend(part.strip() for part in str(row[k]).split(CAPTION_SPLIT))
            p = row[img_key]
            paths.append(p if os.path.isabs(p) else os.path.join(base, p))
            captions.append(caps)
    return paths, captions


def main(argv=None):
    ap = argparse.ArgumentParser(description="pack an image-caption table into the uint8 format data.PackedLoader reads")
    ap.add_argument("--csv", required=True)
    ap.add_argument("--csv-img-key", default="filepath")
    ap.add_argument("--csv-caption-key", default="title")
    ap.add_argument("--csv-separator", default="\t")
    ap.add_argument("--model", required=True, help="selects the tokenizer: get_tokenizer(NAME)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--max-side", type=int, default=None)
    a = ap.parse_args(argv)
    from .factory import get_tokenizer
    paths, captions = read_csv(a.csv, a.csv_img_key, a.csv_caption_key, a.csv_separator)
    tokenizer = get_tokenizer(a.model)
    meta = write_packed(a.out, (decode_rgb(p, a.max_side) for p in paths), captions, tokenizer,
                        tokenizer_name=f"{type(tokenizer).__name__}:{a.model}")
    print(json.dumps(meta))
    return 0


if __name__ == "__main__":
    sys.exit(main())
