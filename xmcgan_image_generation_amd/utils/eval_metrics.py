"""FID and Inception Score of a generator (the reference's ``xmcgan/utils/eval_metrics.py``, its ``test`` mode).

``EvalMetric`` mirrors the reference's class: the real images' Inception pools are computed once in the constructor
(``eval_num // eval_batch_size + 1`` batches of ``next(ds)["image"]``, truncated to ``eval_num``);
``calculate_inception_fid`` runs ``eval_avg_num`` passes over as many batches of generated images -- from the current and
from the EMA generator parameters, ``train_utils.eval_step`` -- and returns the 8-tuple
``(fid, fid_std, is, is_std, ema_fid, ema_fid_std, ema_is, ema_is_std)`` (mean and std over the passes).

Seeds.  The reference draws z with ``jax.random.fold_in(fold_in(rng, pass), step)``, split over the local devices.  Here
the z of pass ``i``, batch ``step`` on rank ``r`` comes from ``torch.Generator().manual_seed(seed)`` (inside ``eval_step``)
with ``seed = SeedSequence([rng, i, step, r]).generate_state(1, uint64)[0] >> 1``: a pure function of ``(rng, pass, step,
rank)``, so two calls with the same ``rng`` see the same z.

Batching.  Images are buffered so that Inception runs on chunks of ``chunk`` images whatever ``eval_batch_size`` is (at the
reference's 7 images per batch the 8 x 8 layers would fill a few of the 256 CUs).  The kernels' summation order does not
depend on the chunk, so an image's pool is the same however the evaluation batches it.

With a ``group`` (``torch.distributed``), every rank draws its own batches, and pools and predictions are all-gathered in
rank-major order before truncation -- the reference's ``lax.all_gather`` + reshape: every rank returns the same numbers.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import alignment_metrics, inception_utils, sample_metrics

# config.eval_extra_metrics: name -> the keys ``EvalMetric.calculate_metrics`` adds for it (mean and std over the passes)
EXTRA_METRIC_KEYS = {
    "kid": ("kid", "kid_std", "ema_kid", "ema_kid_std"),
    "precision_recall": ("precision", "precision_std", "recall", "recall_std",
                         "ema_precision", "ema_precision_std", "ema_recall", "ema_recall_std"),
    # text-image alignment on CLIP embeddings (utils/alignment_metrics.py).  real_*: the real images against their own captions,
    # computed once per EvalMetric -- the ceiling the generated scores are read against (no std: there is one pass of it)
    "clip": ("clip_score", "clip_score_std", "r_precision", "r_precision_std", "ema_clip_score", "ema_clip_score_std",
             "ema_r_precision", "ema_r_precision_std", "real_clip_score", "real_r_precision"),
}


def extra_metric_keys(names):
    """the keys ``calculate_metrics`` returns beyond the eight of FID / IS for ``config.eval_extra_metrics = names``"""
    unknown = [n for n in names if n not in EXTRA_METRIC_KEYS]
    if unknown:
        raise ValueError(f"eval_extra_metrics: unknown name(s) {unknown}; known: {sorted(EXTRA_METRIC_KEYS)}")
    return tuple(k for n in sorted(set(names)) for k in EXTRA_METRIC_KEYS[n])


def batch_seed(rng, pass_index, step, rank=0):
    """the integer seed of generated batch ``step`` of pass ``pass_index`` on ``rank`` (module docstring)"""
    state = np.random.SeedSequence([int(rng) & 0xFFFFFFFFFFFFFFFF, int(pass_index), int(step), int(rank)])
    return int(state.generate_state(1, np.uint64)[0] >> np.uint64(1))


def _captions(batch):
    """the caption texts of a batch as strings (``COCODataset(return_caption_text=True)`` / ``return_text`` put bytes there)"""
    if "text" not in batch:
        raise ValueError('eval_extra_metrics "clip" needs the captions\' text in every evaluation batch (batch["text"]: '
                         "COCODataset(return_caption_text=True), which create_datasets sets when \"clip\" is requested)")
    return [c.decode("utf-8") if isinstance(c, bytes) else str(c) for c in batch["text"]]


def _images(x):
    return x.detach().float() if isinstance(x, torch.Tensor) else np.asarray(x, np.float32)


class _Chunker:
    """collects images and runs ``inception`` on full chunks of ``chunk`` images (the tail on what is left)"""

    def __init__(self, inception, chunk):
        self.inception, self.chunk = inception, int(chunk)
        self.pending, self.count, self.pools, self.preds = [], 0, [], []

    def add(self, images):
        self.pending.append(images)
        self.count += images.shape[0]
        while self.count >= self.chunk:
            self._run(self.chunk)

    def _run(self, n):
        take, left, got = [], [], 0
        for im in self.pending:
            if got >= n:
                left.append(im)
                continue
            k = min(n - got, im.shape[0])
            take.append(im[:k])
            if k < im.shape[0]:
                left.append(im[k:])
            got += k
        self.pending, self.count = left, self.count - got
        if isinstance(take[0], torch.Tensor):
            images = take[0] if len(take) == 1 else torch.cat(take, 0)
        else:
            images = take[0] if len(take) == 1 else np.concatenate(take, 0)
        pool, preds = self.inception(images)
        self.pools.append(np.asarray(pool, np.float32))
        self.preds.append(np.asarray(preds, np.float32))

    def finish(self):
        if self.count:
            self._run(self.count)
        return np.concatenate(self.pools, 0), np.concatenate(self.preds, 0)


class EvalMetric:
    """FID / Inception Score evaluation (eval_metrics.py:31-216).

    ``ds``: iterator of batches (``next(ds)["image"]`` (B, H, W, 3) in [0, 1], plus the caption fields ``eval_step`` needs);
    ``config``: ``eval_num``, ``eval_batch_size``, ``eval_avg_num``; ``inception_ckpt_path``: see
    ``inception_utils.inception_model`` (``None`` = random weights, whose FID means nothing); ``ops``: a ``HipOps`` (default: a
    new one in ``dtype``); ``dtype``: float32 as the reference, bf16 opt-in; ``inception``: any callable
    ``images -> (pool, preds)`` in place of the HIP network; ``chunk``: images per Inception launch sequence; ``group``: a
    ``torch.distributed`` process group; ``metric_ops``: the operator table of the extra metrics (``calculate_metrics``; default:
    the table Inception runs on, or none -- the NumPy specification -- beside an injected ``inception``); ``clip``: with ``"clip"``
    in ``config.eval_extra_metrics``, any object with ``embed_text(list of str) -> (n, d)`` and ``embed_image(images) -> (n, d)`` in
    place of the ``clip_utils.ClipScorer`` built from ``config.clip_vocab_path`` / ``clip_merges_path`` / ``clip_ckpt_path`` /
    ``clip_fast`` (ignored without ``"clip"``)."""

    def __init__(self, ds, config, num_splits=1, inception_ckpt_path=None, *, ops=None, dtype=torch.float32, inception=None,
                 chunk=256, group=None, metric_ops=None, clip=None):
        self.ds = ds
        self.config = config
        self.eval_num = int(config.eval_num)
        self.eval_batch_size = int(config.eval_batch_size)
        self.avg_num = int(config.eval_avg_num)
        self.num_splits = num_splits
        self.chunk = chunk
        self.group = group
        if inception is None:
            if inception_ckpt_path is None:
                warnings.warn("EvalMetric: random Inception-v3 weights (inception_ckpt_path=None): FID and IS from them mean "
                              "nothing; convert the real weights and pass their path", stacklevel=2)
            if ops is None:
                from ..ops import HipOps
                ops = HipOps(dtype=dtype)
            state = inception_utils.inception_model(inception_ckpt_path)
            inception = inception_utils.InceptionV3Features(ops, state["params"], state["batch_stats"])
        self.inception = inception
        self.metric_ops = metric_ops if metric_ops is not None else ops
        self._real_radii = {}                     # pr_k -> k-NN radii of the real pool (it never changes)
        self.clip = None
        if "clip" in tuple(config.get("eval_extra_metrics", ())):
            self.clip = clip if clip is not None else self._make_clip(ops)
        self.real_alignment = {}                  # real_clip_score / real_r_precision, filled with the real pool
        self._pool = self._get_real_pool_for_evaluation()

    @property
    def n_iter(self):
        return self.eval_num // self.eval_batch_size + 1

    def _rank(self):
        if self.group is None:
            return 0
        import torch.distributed as dist
        return dist.get_rank(self.group)

    def _gather(self, a):
        """all-gather an (n, d) array over the group, rank-major (the reference's all_gather + reshape)"""
        if self.group is None:
            return a
        import torch.distributed as dist
        world = dist.get_world_size(self.group)
        dev = torch.device("cpu") if dist.get_backend(self.group) == "gloo" else torch.device("cuda", torch.cuda.current_device())
        t = torch.as_tensor(np.ascontiguousarray(a)).to(dev)
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t, group=self.group)
        return np.concatenate([p.cpu().numpy() for p in parts], 0)

    def _make_clip(self, ops):
        from . import clip_utils
        cfg = self.config
        fast = bool(cfg.get("clip_fast", False))
        if cfg.get("clip_ckpt_path", None) is None:
            warnings.warn("EvalMetric: random CLIP weights (clip_ckpt_path=None): CLIPScore and R-precision from them mean "
                          "nothing; convert the real weights and pass their path", stacklevel=3)
        if ops is not None and fast and ops.dtype != torch.bfloat16:
            ops = None                            # the bf16 GEMMs of the fast mode need the bf16 table: the scorer makes one
        return clip_utils.ClipScorer(cfg.clip_vocab_path, cfg.clip_merges_path, cfg.get("clip_ckpt_path", None), ops=ops, fast=fast,
                                     chunk=self.chunk)

    def _alignment(self, img, txt, seed):
        """(clip_score, r_precision) of paired embedding lists, gathered over the group and truncated to ``eval_num``; the
        candidates come from ``seed``"""
        img = self._gather(np.concatenate(img, 0).astype(np.float32))[:self.eval_num]
        txt = self._gather(np.concatenate(txt, 0).astype(np.float32))[:self.eval_num]
        cand = alignment_metrics.draw_candidates(seed, img.shape[0], int(self.config.get("r_precision_candidates", 99)))
        return (alignment_metrics.clip_score(img, txt, self.metric_ops), alignment_metrics.r_precision(img, txt, cand, self.metric_ops))

    def _finish(self, chunker):
        pool, preds = chunker.finish()
        return self._gather(pool)[:self.eval_num], self._gather(preds)[:self.eval_num]

    def _get_real_pool_for_evaluation(self):
        ch = _Chunker(self.inception, self.chunk)
        img, txt = [], []
        for _ in range(self.n_iter):
            batch = next(self.ds)
            ch.add(_images(batch["image"]))
            if self.clip is not None:
                img.append(np.asarray(self.clip.embed_image(_images(batch["image"])), np.float32))
                txt.append(np.asarray(self.clip.embed_text(_captions(batch)), np.float32))
        pool, _ = self._finish(ch)
        if self.clip is not None:
            seed = np.random.SeedSequence([int(self.config.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF, alignment_metrics.CLIP_SALT])
            score, rprec = self._alignment(img, txt, seed)
            self.real_alignment = {"real_clip_score": score, "real_r_precision": rprec}
        return pool

    def _get_generated_pool_for_evaluation(self, generator_fn, state, rng):
        from .. import train_utils
        ch, ema_ch = _Chunker(self.inception, self.chunk), _Chunker(self.inception, self.chunk)
        rank = self._rank()
        pass_index, pass_rng = rng
        self._pass_embeddings = emb = {"img": [], "ema_img": [], "txt": []}      # read by calculate_metrics ("clip")
        for step in range(self.n_iter):
            batch = next(self.ds)
            seed = batch_seed(pass_rng, pass_index, step, rank)
            image, ema_image = train_utils.eval_step(seed, state, batch, generator_fn, self.config)
            ch.add(_images(image))
            ema_ch.add(_images(ema_image))
            if self.clip is not None:             # encoded as the batches come: no image is kept
                emb["img"].append(np.asarray(self.clip.embed_image(_images(image)), np.float32))
                emb["ema_img"].append(np.asarray(self.clip.embed_image(_images(ema_image)), np.float32))
                emb["txt"].append(np.asarray(self.clip.embed_text(_captions(batch)), np.float32))
        pool, preds = self._finish(ch)
        ema_pool, ema_preds = self._finish(ema_ch)
        return pool, preds, ema_pool, ema_preds

    def calculate_inception_fid(self, generator_fn, state, rng):
        """-> (fid, fid_std, inception_score, inception_score_std, ema_fid, ema_fid_std, ema_inception_score,
        ema_inception_score_std): mean and std over ``eval_avg_num`` passes (eval_metrics.py:172-216)"""
        fid_list, is_list, ema_fid_list, ema_is_list = [], [], [], []
        for i in range(self.avg_num):
            pool, preds, ema_pool, ema_preds = self._get_generated_pool_for_evaluation(generator_fn, state, (i, rng))
            is_list.append(inception_utils.calculate_inception_score(preds, num_splits=self.num_splits)[0])
            ema_is_list.append(inception_utils.calculate_inception_score(ema_preds, num_splits=self.num_splits)[0])
            fid_list.append(inception_utils.calculate_fid(pool, self._pool))
            ema_fid_list.append(inception_utils.calculate_fid(ema_pool, self._pool))
        return (float(np.mean(fid_list)), float(np.std(fid_list)), float(np.mean(is_list)), float(np.std(is_list)),
                float(np.mean(ema_fid_list)), float(np.std(ema_fid_list)), float(np.mean(ema_is_list)), float(np.std(ema_is_list)))

    def real_radii(self, k):
        """squared k-NN radii of the real pool, computed once per ``EvalMetric`` and ``k``"""
        if k not in self._real_radii:
            self._real_radii[k] = sample_metrics.knn_radii(self._pool, k, self.metric_ops)
        return self._real_radii[k]

    def calculate_metrics(self, generator_fn, state, rng):
        """-> dict: the eight values of ``calculate_inception_fid`` under their ``train_utils.EVAL_KEYS`` names (the same pools, the same
        arithmetic: bit-equal for the same ``rng``) and, for every name in ``config.eval_extra_metrics``, the mean and std over the
        passes of KID (``kid``, ``kid_std``) and / or improved precision and recall (``precision``, ``precision_std``, ``recall``,
        ``recall_std``), each also from the EMA parameters (``ema_`` prefix).  Both are computed from the pools FID uses
        (``utils/sample_metrics.py``).  The KID subsets of pass i are drawn from ``SeedSequence([rng, i, 0x4B4944])`` and are the same
        for the current and the EMA pool.  ``"clip"`` adds CLIPScore and R-precision of the generated images against the captions
        they were generated from (``utils/alignment_metrics.py``; the candidates of pass i from ``SeedSequence([rng, i,
        0x434C4950])``, the same for the current and the EMA images) and ``real_clip_score`` / ``real_r_precision``, the same two
        scores of the real images against their own captions."""
        cfg = self.config
        extras = tuple(cfg.get("eval_extra_metrics", ()))
        extra_metric_keys(extras)
        if "clip" in extras and self.clip is None:
            raise ValueError('eval_extra_metrics names "clip" but this EvalMetric was built without it')
        lists = {k: [] for k in ("fid", "is", "ema_fid", "ema_is", "kid", "ema_kid", "precision", "recall", "ema_precision",
                                 "ema_recall", "clip_score", "r_precision", "ema_clip_score", "ema_r_precision")}
        for i in range(self.avg_num):
            pool, preds, ema_pool, ema_preds = self._get_generated_pool_for_evaluation(generator_fn, state, (i, rng))
            lists["is"].append(inception_utils.calculate_inception_score(preds, num_splits=self.num_splits)[0])
            lists["ema_is"].append(inception_utils.calculate_inception_score(ema_preds, num_splits=self.num_splits)[0])
            lists["fid"].append(inception_utils.calculate_fid(pool, self._pool))
            lists["ema_fid"].append(inception_utils.calculate_fid(ema_pool, self._pool))
            for prefix, p in (("", pool), ("ema_", ema_pool)):
                if "kid" in extras:
                    seed = np.random.SeedSequence([int(rng) & 0xFFFFFFFFFFFFFFFF, i, sample_metrics.KID_SALT])
                    lists[prefix + "kid"].append(sample_metrics.kid(p, self._pool, int(cfg.get("kid_subsets", 100)),
                                                                    int(cfg.get("kid_subset_size", 1000)), seed, self.metric_ops)[0])
                if "precision_recall" in extras:
                    k = int(cfg.get("pr_k", 3))
                    pr = sample_metrics.precision_recall(p, self._pool, k, self.metric_ops, real_radii=self.real_radii(k))
                    lists[prefix + "precision"].append(pr[0])
                    lists[prefix + "recall"].append(pr[1])
            if "clip" in extras:
                emb = self._pass_embeddings
                for prefix in ("", "ema_"):
                    seed = np.random.SeedSequence([int(rng) & 0xFFFFFFFFFFFFFFFF, i, alignment_metrics.CLIP_SALT])
                    score, rprec = self._alignment(emb[prefix + "img"], emb["txt"], seed)
                    lists[prefix + "clip_score"].append(score)
                    lists[prefix + "r_precision"].append(rprec)
        out = {}
        for key, name in (("fid", "fid"), ("inception_score", "is"), ("ema_fid", "ema_fid"), ("ema_inception_score", "ema_is")):
            out[key], out[key + "_std"] = float(np.mean(lists[name])), float(np.std(lists[name]))
        for key in extra_metric_keys(extras):
            if key in self.real_alignment:
                out[key] = float(self.real_alignment[key])
            elif not key.endswith("_std"):
                out[key], out[key + "_std"] = float(np.mean(lists[key])), float(np.std(lists[key]))
        return out
