"""Synthetic data branch the reference's main.py tests for but data.py never built
(reference main.py:277 vs data.py:185-189).  Batch contract of the
reference loader: (images[B,3,H,W] float, texts[B,K,77] int64) with texts[:,0] used
(reference data.py:306-312, train.py:121-122) and dataloader.num_batches/.num_samples.

`--dataset-type packed` is the real-image path: a directory written once by `python -m colxlip_amd.pack` (raw uint8 images,
token ids), read here through `np.memmap`; the host only gathers bytes, the crop / resample / normalise of the reference's
image_transform_v2 (reference factory.py:411-418) runs on the device (`image_transform.DeviceImageTransform`)."""
import json
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch


def synthetic_batch(batch, image_size, context_length=77, vocab_size=49408, seed=1234, device="cpu",
                    image_dtype=torch.float32, captions_per_image=1):
    """images ~ N(0,1); ids U[1, vocab-2), one EOT (= vocab-1) per row at a random position in
    [8, L-1], zeros after it.  Same RNG recipe as oracle.clip_oracle.synthetic_batch."""
    g = torch.Generator().manual_seed(seed)
    hw = image_size if isinstance(image_size, (tuple, list)) else (image_size, image_size)
    images = torch.randn(batch, 3, hw[0], hw[1], generator=g)
    L = context_length
    text = torch.randint(1, vocab_size - 2, (batch, L), generator=g)
    eot = torch.randint(min(8, L - 1), L, (batch,), generator=g)
    pos = torch.arange(L).unsqueeze(0)
    text = torch.where(pos < eot.unsqueeze(1), text, torch.zeros_like(text))
    text[torch.arange(batch), eot] = vocab_size - 1
    texts = text.unsqueeze(1).expand(batch, captions_per_image, L).contiguous()
    return images.to(device=device, dtype=image_dtype), texts.to(device)


class SyntheticLoader:
    """Iterates `num_batches` device-resident batches (a small pool, cycled)."""

    def __init__(self, batch_size, num_samples, image_size, context_length, vocab_size, device, world_size=1,
                 rank=0, seed=1234, pool=2, image_dtype=torch.float32):
        self.batch_size = batch_size
        self.num_samples = num_samples
        self.num_batches = max(1, num_samples // (batch_size * world_size))
        self._pool = [synthetic_batch(batch_size, image_size, context_length, vocab_size,
                                      seed=seed + 1000 * rank + i, device=device, image_dtype=image_dtype)
                      for i in range(pool)]

    def __len__(self):
        return self.num_batches

    def __iter__(self):
        for i in range(self.num_batches):
            yield self._pool[i % len(self._pool)]


@dataclass
class DataInfo:
    dataloader: SyntheticLoader
    sampler: Optional[object] = None
    shared_epoch: Optional[object] = None

    def set_epoch(self, epoch):
        if hasattr(self.dataloader, "set_epoch"):
            self.dataloader.set_epoch(epoch)


class _IdLoader:
    """Batches of (tensor, ids) over a fixed tensor: the two loaders of a retrieval split (reference data.py:1133-1178)."""

    def __init__(self, items, ids, batch_size):
        self.items, self.ids, self.batch_size = items, ids, batch_size
        self.num_samples = len(ids)
        self.num_batches = (len(ids) + batch_size - 1) // batch_size

    def __len__(self):
        return self.num_batches

    def __iter__(self):
        for lo in range(0, self.num_samples, self.batch_size):
            yield self.items[lo:lo + self.batch_size], self.ids[lo:lo + self.batch_size]


def synthetic_retrieval_split(num_images, captions_per_image, image_size, context_length=77, vocab_size=49408, seed=4321,
                              device="cpu", batch_size=64, image_dtype=torch.float32):
    """A retrieval split in the reference's shape: (text DataInfo, image DataInfo, img2txt_dict, txt2img_dict), COCO-like
    (`captions_per_image` captions per image).  Caption ids enumerate the text rows; image ids are arbitrary dataset numbers
    in shuffled order, so the id -> row remapping of the eval loop is exercised (reference train.py:429-454)."""
    n_txt = num_images * captions_per_image
    images, _ = synthetic_batch(num_images, image_size, context_length, vocab_size, seed=seed, device=device, image_dtype=image_dtype)
    _, texts = synthetic_batch(n_txt, 8, context_length, vocab_size, seed=seed + 1, device=device)
    g = torch.Generator().manual_seed(seed + 2)
    img_ids = (1000 + 7 * torch.randperm(num_images, generator=g)).to(torch.int64)
    cap_ids = torch.arange(n_txt, dtype=torch.int64)
    owner = torch.arange(n_txt) // captions_per_image                   # caption row -> image row
    img2txt = {int(img_ids[i]): [int(c) for c in cap_ids[owner == i]] for i in range(num_images)}
    txt2img = {int(c): [int(img_ids[owner[c]])] for c in range(n_txt)}
    txt_loader = _IdLoader(texts[:, 0].contiguous(), cap_ids, batch_size)
    img_loader = _IdLoader(images, img_ids, batch_size)
    return DataInfo(dataloader=txt_loader), DataInfo(dataloader=img_loader), img2txt, txt2img


# ------------------------------------------------------------------ packed uint8 dataset (written by colxlip_amd.pack)
_STAGE_ALIGN = 256


def _round_up(n, a):
    return (n + a - 1) // a * a


def _seed_of(*key) -> int:
    """one 63-bit seed from a tuple of small integers, e.g. (seed, epoch, rank, batch)"""
    return int(np.random.SeedSequence([int(k) for k in key]).generate_state(1, np.uint64)[0] >> np.uint64(1))


class PackedDataset:
    """Read side of a packed directory: `images` (uint8 memmap), `index` int64 [n, 3] (offset, h, w), `tokens` int32 [n, K, L]."""

    def __init__(self, root):
        from .pack import FILES
        missing = [f for f in FILES if not os.path.exists(os.path.join(root, f))]
        if missing:
            raise FileNotFoundError(f"{root} is not a packed dataset (missing {', '.join(missing)}): write one with "
                                    "python -m colxlip_amd.pack")
        with open(os.path.join(root, "meta.json")) as f:
            self.meta = json.load(f)
        self.root = root
        self.index = np.load(os.path.join(root, "index.npy"))
        self.tokens = np.load(os.path.join(root, "tokens.npy"), mmap_mode="r")
        self.images = np.memmap(os.path.join(root, "images.u8"), dtype=np.uint8, mode="r")
        self.n, self.K, self.context_length = int(self.meta["n"]), int(self.meta["K"]), int(self.meta["context_length"])
        if self.index.shape != (self.n, 3) or self.tokens.shape != (self.n, self.K, self.context_length):
            raise ValueError(f"{root}: index / tokens do not match meta.json")
        sizes = 3 * self.index[:, 1] * self.index[:, 2]
        if self.n and (self.index[:, 0].min() < 0 or int((self.index[:, 0] + sizes).max()) > self.images.size):
            raise ValueError(f"{root}: index.npy points outside images.u8")

    def __len__(self):
        return self.n

    def image(self, i) -> np.ndarray:
        off, h, w = (int(v) for v in self.index[i])
        return self.images[off:off + 3 * h * w].reshape(h, w, 3)


class _Staged:
    """One staged batch: where its images, records and token ids lie in the staging buffer."""
    __slots__ = ("slot", "idx", "n", "meta_bytes", "tok_off", "tok_bytes", "img_off", "total", "futures")


class _PackedStream:
    """Device-resident image batches from a PackedDataset.  Per batch: the images' bytes, the kernel's records and the token ids are
    gathered into one of two pinned staging buffers on at most `workers` threads, copied to one of two device buffers on a copy
    stream, and transformed on the consumer's stream.  The gather of batch k+1 is started before batch k is handed out, so it and
    its copy overlap batch k's consumption.  Reuse is ordered by events, never a device-wide sync: a staging buffer is refilled
    only after the copy that read it has finished (`_copied`, waited for on the host), a device buffer is overwritten only after
    the transform that read it has finished (`_consumed`, waited for by the copy stream)."""

    def __init__(self, ds, transform, device, image_dtype, workers):
        self.ds, self.transform, self.device, self.image_dtype = ds, transform, torch.device(device), image_dtype
        self.workers = max(1, int(workers))
        self._pool = None
        self._stage = [None, None]
        self._raw = [None, None]
        self._copied = [None, None]
        self._consumed = [None, None]
        self._copy_stream = None

    def _start(self, k, idx, generator):
        """plan batch number k (images idx, in this order) into staging slot k % 2 and start its gather"""
        ds, st = self.ds, _Staged()
        st.slot, st.idx, st.n = k % 2, np.asarray(idx, dtype=np.int64), len(idx)
        rows = ds.index[st.idx]
        sizes = 3 * rows[:, 1] * rows[:, 2]
        st.meta_bytes = _round_up(48 * st.n, _STAGE_ALIGN)
        st.tok_off, st.tok_bytes = st.meta_bytes, 4 * st.n * ds.K * ds.context_length
        st.img_off = st.tok_off + _round_up(st.tok_bytes, _STAGE_ALIGN)
        padded = (sizes + 63) // 64 * 64
        dst = np.concatenate([[0], np.cumsum(padded)[:-1]]) if st.n else np.zeros(0, dtype=np.int64)
        img_bytes = int(padded.sum())
        st.total = st.img_off + img_bytes
        meta = self.transform.geometry(torch.from_numpy(dst), torch.from_numpy(rows[:, 1:3].copy()), img_bytes, generator)
        if self._copied[st.slot] is not None:
            self._copied[st.slot].synchronize()            # the copy that last read this staging buffer
        if self._stage[st.slot] is None or self._stage[st.slot].numel() < st.total:
            self._stage[st.slot] = torch.empty(_round_up(int(st.total * 1.25), 1 << 20), dtype=torch.uint8, pin_memory=True)
        stage = self._stage[st.slot].numpy()
        stage[:48 * st.n] = meta.numpy().view(np.uint8).reshape(-1)
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.workers)
        images, tokens = ds.images, ds.tokens
        src = rows[:, 0]

        def gather(lo, hi):
            for j in range(lo, hi):
                a, b = st.img_off + int(dst[j]), int(src[j])
                stage[a:a + int(sizes[j])] = images[b:b + int(sizes[j])]
            tok = stage[st.tok_off:st.tok_off + st.tok_bytes].view(np.int32).reshape(st.n, ds.K, ds.context_length)
            for j in range(lo, hi):
                tok[j] = tokens[int(st.idx[j])]

        per = -(-st.n // self.workers) if st.n else 1
        st.futures = [self._pool.submit(gather, lo, min(st.n, lo + per)) for lo in range(0, st.n, per)]
        return st

    def _finish(self, st):
        """staging -> device (copy stream) -> (images [n,3,H,W], tokens int64 [n,K,L]) on the current stream"""
        for f in st.futures:
            f.result()
        main = torch.cuda.current_stream(self.device)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        if self._raw[st.slot] is None or self._raw[st.slot].numel() < st.total:
            self._raw[st.slot] = torch.empty(self._stage[st.slot].numel(), dtype=torch.uint8, device=self.device)
            self._copy_stream.wait_stream(main)            # a fresh buffer: ordered behind whatever used this memory before
        raw = self._raw[st.slot]
        with torch.cuda.stream(self._copy_stream):
            if self._consumed[st.slot] is not None:
                self._copy_stream.wait_event(self._consumed[st.slot])
            raw[:st.total].copy_(self._stage[st.slot][:st.total], non_blocking=True)
            self._copied[st.slot] = torch.cuda.Event()
            self._copied[st.slot].record(self._copy_stream)
        main.wait_event(self._copied[st.slot])
        meta = raw[:48 * st.n].view(torch.int64).view(st.n, 6)
        images = self.transform(raw[st.img_off:st.total], meta, self.image_dtype)
        ds = self.ds
        texts = raw[st.tok_off:st.tok_off + st.tok_bytes].view(torch.int32).view(st.n, ds.K, ds.context_length).to(torch.int64)
        self._consumed[st.slot] = torch.cuda.Event()
        self._consumed[st.slot].record(main)
        return images, texts

    def batches(self, plans):
        """plans: list of (image indices, generator or None); yields (images, texts) per plan, one gather ahead"""
        pending = self._start(0, *plans[0]) if plans else None
        try:
            for k in range(len(plans)):
                st = pending
                for f in st.futures:                       # batch k is gathered before k+1 may take the threads
                    f.result()
                pending = self._start(k + 1, *plans[k + 1]) if k + 1 < len(plans) else None
                yield self._finish(st)
        finally:                                           # an abandoned iteration leaves no gather writing into a staging buffer
            for f in (pending.futures if pending is not None else ()):
                f.result()


class PackedLoader:
    """Train loader over a packed directory with the batch contract of the reference's loaders: iterating yields device-resident
    (images [B,3,H,W] in `image_dtype`, texts [B,K,L] int64); `.num_batches`, `.num_samples`.  Epoch e walks a permutation seeded
    by (seed, e); rank r takes perm[r::world_size], truncated so that every rank makes the same number of full batches.  The crop
    boxes of batch k come from a generator seeded by (seed, epoch, rank, k)."""

    def __init__(self, root, batch_size, transform, device, image_dtype=torch.float32, world_size=1, rank=0, seed=0, workers=4):
        self.ds = root if isinstance(root, PackedDataset) else PackedDataset(root)
        self.batch_size, self.world_size, self.rank, self.seed = int(batch_size), int(world_size), int(rank), int(seed)
        self.transform = transform
        self.num_samples = len(self.ds)
        self.num_batches = (len(self.ds) // self.world_size) // self.batch_size
        if self.num_batches < 1:
            raise ValueError(f"{self.ds.root}: {len(self.ds)} images do not fill one batch of {self.batch_size} on each of "
                             f"{self.world_size} ranks")
        self.epoch = 0
        self._stream = _PackedStream(self.ds, transform, device, image_dtype, workers)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.num_batches

    def order(self, epoch=None) -> np.ndarray:
        """this rank's image indices of an epoch, [num_batches * batch_size]"""
        epoch = self.epoch if epoch is None else int(epoch)
        perm = np.random.default_rng(np.random.SeedSequence([self.seed, epoch])).permutation(len(self.ds))
        return perm[self.rank::self.world_size][:self.num_batches * self.batch_size]

    def batch_generator(self, epoch, k) -> torch.Generator:
        return torch.Generator().manual_seed(_seed_of(self.seed, epoch, self.rank, k))

    def plan(self, epoch=None):
        """[(image indices, box generator)] of an epoch's batches"""
        epoch = self.epoch if epoch is None else int(epoch)
        order = self.order(epoch)
        return [(order[k * self.batch_size:(k + 1) * self.batch_size], self.batch_generator(epoch, k))
                for k in range(self.num_batches)]

    def __iter__(self):
        return self._stream.batches(self.plan())


class _PackedImageIdLoader:
    """Image side of a retrieval split over a packed directory: every image once, in order, through the val transform; yields
    (images, image ids) with the image's row in the dataset as its id."""

    def __init__(self, ds, batch_size, transform, device, image_dtype, workers):
        self.ds, self.batch_size = ds, int(batch_size)
        self.num_samples = len(ds)
        self.num_batches = (len(ds) + self.batch_size - 1) // self.batch_size
        self._stream = _PackedStream(ds, transform, device, image_dtype, workers)

    def __len__(self):
        return self.num_batches

    def __iter__(self):
        plans = [(np.arange(lo, min(len(self.ds), lo + self.batch_size)), None) for lo in range(0, len(self.ds), self.batch_size)]
        for (idx, _), (images, _texts) in zip(plans, self._stream.batches(plans)):
            yield images, torch.from_numpy(idx)


def packed_retrieval_split(root, transform, device, batch_size=64, image_dtype=torch.float32, workers=4):
    """(text DataInfo, image DataInfo, img2txt_dict, txt2img_dict) over a packed directory, the shape `train.evaluate` reads
    (reference data.py:1133-1178): image ids are dataset rows, caption ids enumerate the n*K caption rows, image i owns
    captions i*K .. i*K+K-1."""
    ds = root if isinstance(root, PackedDataset) else PackedDataset(root)
    n, K = len(ds), ds.K
    texts = torch.from_numpy(np.ascontiguousarray(ds.tokens).reshape(n * K, ds.context_length).astype(np.int64)).to(device)
    cap_ids = torch.arange(n * K, dtype=torch.int64)
    img2txt = {i: list(range(i * K, i * K + K)) for i in range(n)}
    txt2img = {c: [c // K] for c in range(n * K)}
    txt_loader = _IdLoader(texts, cap_ids, batch_size)
    img_loader = _PackedImageIdLoader(ds, batch_size, transform, device, image_dtype, workers)
    return DataInfo(dataloader=txt_loader), DataInfo(dataloader=img_loader), img2txt, txt2img


def _image_size_from(preprocess_fns, model):
    if model is not None:
        return model.visual.image_size
    for fn in preprocess_fns or ():
        size = getattr(getattr(fn, "cfg", None), "size", None)
        if size is not None:
            return size
    return 224


def get_data(args, preprocess_fns=None, epoch=0, tokenizer=None, model=None):
    """reference data.py:191-232 -- the synthetic branch, and `packed` (`_get_packed_data`: images decoded and captions
    tokenised once, offline, by `python -m colxlip_amd.pack`; file/tar IO and JPEG decode at train time are not built).  The reference's call `get_data(args, (preprocess_train, preprocess_val), epoch=,
    tokenizer=)` works: image size comes from the transforms the factory returned (or from `model=` when given).
    `--retrieval-coco` / `--retrieval-flickr` add a synthetic retrieval split under the reference's key (`--val-num-samples`
    images, 5 captions each) for `train.evaluate`."""
    if args.dataset_type == "packed":
        return _get_packed_data(args, preprocess_fns, model)
    if args.dataset_type != "synthetic":
        raise ValueError(f"Unsupported dataset type: {args.dataset_type} (this stack provides 'synthetic' and 'packed')")
    image_size = _image_size_from(preprocess_fns, model)
    ctx_len = getattr(model, "context_length", 77)
    vocab = getattr(model, "vocab_size", 49408)
    data = {}
    if args.train_data or args.train_num_samples or not (args.retrieval_coco or args.retrieval_flickr):
        n = args.train_num_samples or args.batch_size * args.world_size * 100
        loader = SyntheticLoader(args.batch_size, n, image_size, ctx_len, vocab, args.device,
                                 world_size=args.world_size, rank=args.rank, seed=1234 + args.seed)
        data["train"] = DataInfo(dataloader=loader)
    for flag, key, seed in (("retrieval_coco", "retrieval_coco", 4321), ("retrieval_flickr", "retrieval_flickr", 8765)):
        if getattr(args, flag, False):
            data[key] = synthetic_retrieval_split(getattr(args, "val_num_samples", None) or 4 * args.batch_size, 5, image_size,
                                                  ctx_len, vocab, seed=seed + args.seed, device=args.device,
                                                  batch_size=args.batch_size)
    return data


def _get_packed_data(args, preprocess_fns, model):
    """`--dataset-type packed`: `--train-data DIR` gives data["train"] (train transform: random resized crops, `--aug-cfg scale=
    ratio=`); `--retrieval-coco` / `--retrieval-flickr` with `--val-data DIR` give a retrieval split through the val transform."""
    from .image_transform import transform_from
    from .model import get_input_dtype
    size = _image_size_from(preprocess_fns, model)
    size = tuple(size) if isinstance(size, (tuple, list)) else (size, size)
    pre_train, pre_val = (tuple(preprocess_fns) + (None, None))[:2] if preprocess_fns else (None, None)
    # the kernel writes bf16 or fp32; any other input dtype (fp16) is cast from fp32 by the train loop, as for every loader
    dtype = torch.bfloat16 if get_input_dtype(args.precision) == torch.bfloat16 else torch.float32
    workers = max(1, int(getattr(args, "workers", 4) or 1))
    data = {}
    if args.train_data:
        transform = transform_from(pre_train, True, getattr(args, "aug_cfg", None), size)
        loader = PackedLoader(args.train_data, args.batch_size, transform, args.device, image_dtype=dtype,
                              world_size=args.world_size, rank=args.rank, seed=args.seed, workers=workers)
        data["train"] = DataInfo(dataloader=loader)
    for key in ("retrieval_coco", "retrieval_flickr"):
        if getattr(args, key, False):
            if not args.val_data:
                raise ValueError(f"--{key.replace('_', '-')} with --dataset-type packed needs --val-data DIR")
            data[key] = packed_retrieval_split(args.val_data, transform_from(pre_val, False, None, size), args.device,
                                               batch_size=args.batch_size, image_dtype=dtype, workers=workers)
    if not data:
        raise ValueError("--dataset-type packed needs --train-data DIR, or --val-data DIR with a --retrieval-* flag")
    return data
