"""Step orchestration: ``TrainState``, ``create_train_state``, ``train_step``, ``eval_step``.

Mirrors the hot-path part of the reference's ``xmcgan/train_utils.py``: ``TrainState`` (:42-50),
``split_input_dict`` (:69-88), ``train_step`` (:91-130), ``create_train_state`` (:133-193).  The
reference has no ``eval_step``; the generator-only evaluation it performs in ``generate_batch``
(:245-309) / ``eval_metrics.py:90-124`` -- G(train=False) once with the parameters and once with
the EMA parameters -- is exposed here under that name.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Any, Dict, Optional

import torch

from . import synthetic as syn
from . import xmc_gan
from .libml.layers import ParamArena
from .nets import xmc_net


class Optimizer:
    """flax.optim.Optimizer stand-in: ``.target`` is the Flax-layout parameter tree (views of the
    flat arena), ``.state`` exposes the Adam step and moment trees (train_utils.py:181-186)."""

    def __init__(self, arena: ParamArena, lr, beta1, beta2):
        self.arena, self.lr, self.beta1, self.beta2 = arena, lr, beta1, beta2
        self.target = arena.tree()

    @property
    def state(self):
        return {"step": self.arena.opt_step,
                "param_states": {"grad_ema": self.arena.tree(self.arena.m),
                                 "grad_sq_ema": self.arena.tree(self.arena.v)}}


@dataclasses.dataclass
class TrainState:
    """Data structure for checkpointing the model (reference train_utils.py:42-50)."""
    step: int
    g_optimizer: Optimizer
    d_optimizer: Optimizer
    generator_state: Optional[Any]
    discriminator_state: Optional[Any]
    ema_params: Any
    ema_buffer: Any = None          # flat arena behind ema_params (build-side)
    pending: Any = None             # deferred "wait for the D gradient exchange + Adam" of a train_d (multi-GPU only)
    prefetched_g: Any = None        # (batch identity, (image, new batch_stats, tape)) of the next train_g_d's generator forward (train_d)
    guard: Any = None               # config.skip_nonfinite_updates: the NonfiniteGuard (verdict + skip counters in device memory)
    ada: Any = None                 # config.ada_target: the AdaController (p and the controller's counts in device memory)
    lecam: Any = None               # config.lecam_weight: the LecamController (the two anchors in device memory)

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


class _NetFactory:
    """``functools.partial(generator_cls, config=..., dtype=...)`` of the reference
    (train_utils.py:159-161): called with ``train=`` it returns the (cached) network object."""

    def __init__(self, cls, config, dtype, ops, **kw):
        self.cls, self.config, self.dtype, self.ops, self.kw = cls, config, dtype, ops, kw
        self._cache = {}

    def __call__(self, train):
        if train not in self._cache:
            self._cache[train] = self.cls(self.config, train, dtype=self.dtype, ops=self.ops, **self.kw)
        return self._cache[train]


def split_input_dict(input_dict: Dict[str, torch.Tensor], splits: int, axis=0):
    """train_utils.py:69-88 -- zero-copy views."""
    out = [{} for _ in range(splits)]
    for k, v in input_dict.items():
        v = torch.as_tensor(v)
        if v.shape[axis] % splits != 0:              # jnp.split raises too; torch.chunk would silently give ragged parts
            raise ValueError(f"split_input_dict: '{k}' has {v.shape[axis]} rows, not divisible by {splits}")
        for i, part in enumerate(torch.chunk(v, splits, dim=axis)):
            out[i][k] = part
    return out


def create_train_state(config, rng, init_batch=None, ops=None):
    """-> (generator, discriminator, TrainState) (train_utils.py:133-193).  ``rng`` is an integer
    seed; G / D / (unused) z streams are derived from it like the 3-way split of the reference."""
    dtype = torch.bfloat16 if config.dtype == "bfloat16" else torch.float32
    xmc_net.check_config(config)
    from .libml import diff_augment
    diff_augment.parse_policy(config.get("diff_augment", ""))     # ValueError on an unknown part, before anything is allocated
    from .libml import ada as ada_lib
    ada_lib.check_config(config)                     # config.ada_target: a policy to gate, settings inside their domains
    from .libml import lecam as lecam_lib
    lecam_lib.check_config(config)                   # config.lecam_weight / _decay / _start: inside their domains
    from .libml import opt_schedule
    opt_schedule.check_config(config)                # config.lr_schedule / lr_* / ema_ramp / ema_start_step: inside their domains
    ops = ops if ops is not None else xmc_net.make_ops(dtype)
    if config.get("conv_fp8", False):                # BASELINE config #5: MX-fp8 3x3 convolutions (ops.py::_conv_mx8)
        if dtype != torch.bfloat16:
            raise ValueError("config.conv_fp8 needs config.dtype = 'bfloat16' (activations between the fp8 convolutions are bf16)")
        ops.fp8 = True
        # scale rule of the MX quantisers: "next_binade" (default: no saturating block maximum) or "ocp_floor" (OCP MX v1.0 to the letter)
        ops.set_fp8_scale_rule(config.get("fp8_scale_rule", "next_binade"))
        if config.get("conv_fp8_phase", False):      # ... and the "out"-form phase launches on conv_phase_mx8_kernel (XMC_FP8_PHASE_MX=1 too)
            ops.fp8_phase_mx = True
        if config.get("conv_fp8_phase_in", False):   # ... and the "in"-form ones on conv_phase_in_mx8_kernel (XMC_FP8_PHASE_IN_MX=1 too)
            ops.fp8_phase_in_mx = True
    g_kw = {}
    if config.get("batch_norm_group_size", -1) > 0:  # cross-replica BatchNorm groups: built ONCE (dist.new_group is collective)
        from .dp import BNGroups
        g_kw["bn_groups"] = BNGroups(config)
    generator = _NetFactory(xmc_net.Generator, config, dtype, ops, **g_kw)
    discriminator = _NetFactory(xmc_net.Discriminator, config, dtype, ops)
    seed = int(rng)
    g_vars = generator(train=False).init(seed, None)
    d_vars = discriminator(train=False).init(seed + 1, None)
    g_arena, d_arena = g_vars["params"].arena, d_vars["params"].arena
    ema_buffer = g_arena.params.clone()                                   # ema_params = generator_params (:170)
    from .libml import nonfinite_guard
    guard = nonfinite_guard.NonfiniteGuard(ops.device) if nonfinite_guard.enabled(config) else None
    ada = ada_lib.AdaController(ops.device, config) if ada_lib.enabled(config) else None
    lecam = lecam_lib.LecamController(ops.device, config) if lecam_lib.enabled(config) else None
    state = TrainState(
        step=0,
        g_optimizer=Optimizer(g_arena, config.g_lr, config.beta1, config.beta2),
        d_optimizer=Optimizer(d_arena, config.d_lr, config.beta1, config.beta2),
        generator_state={"batch_stats": g_vars["batch_stats"]},
        discriminator_state={"spectral_norm_stats": d_vars["spectral_norm_stats"]},
        ema_params=g_arena.tree(ema_buffer), ema_buffer=ema_buffer, guard=guard, ada=ada, lecam=lecam)
    return generator, discriminator, state


def load_flax_params(state, g_params=None, g_batch_stats=None, d_params=None, d_sn_stats=None):
    """Install Flax-layout trees (numpy / torch leaves) into a TrainState (checkpoints, tests)."""
    ops = state.g_optimizer.arena.ops
    if g_params is not None:
        state.g_optimizer.arena.load_flax(g_params)
        state.ema_buffer.copy_(state.g_optimizer.arena.params)
    if d_params is not None:
        state.d_optimizer.arena.load_flax(d_params)
    new = {}
    if g_batch_stats is not None:
        new["generator_state"] = {"batch_stats": xmc_net._tree_to_dev(ops, g_batch_stats)}
    if d_sn_stats is not None:
        new["discriminator_state"] = {"spectral_norm_stats": xmc_net._tree_to_dev(ops, d_sn_stats)}
    return state.replace(**new)


def train_step(rng, state, batch, gan_model=xmc_gan, generator=None, discriminator=None, config=None,
               additional_data=None, grad_sync=None, d_aug_host=None):
    """One G+D training step (train_utils.py:91-130): the per-device batch (leading dim
    B * d_step_per_g_step) is split; ``train_d`` runs on the first halves, ``train_g_d`` on the last.
    ``d_aug_host`` (config.diff_augment): the host copy of ``batch["d_aug"]`` when that is a device tensor the caller cannot have
    read back here (``GraphedTrainStep``'s capture); otherwise it is made from the batch."""
    n = config.d_step_per_g_step
    xmc_gan.check_replica_controllers(config, grad_sync)
    if grad_sync is not None and config.get("batch_norm_group_size", -1) > 0:
        grad_sync.require_groups(generator(train=True).bn_groups)
    parts = split_input_dict(batch, n)
    if config.get("diff_augment", "") and "d_aug" in batch and gan_model is xmc_gan:
        # the plan's host copy rides with each half step's rows: the library validates it before the augmentation launches
        host = torch.as_tensor(d_aug_host if d_aug_host is not None else xmc_gan.plan_host_of(batch["d_aug"]))
        for part, rows in zip(parts, torch.chunk(host, n, dim=0)):
            part["d_aug_host"] = rows
    rngs = [int(rng) * n + i for i in range(n)]      # one stream per half step (train_utils.py:121 splits the key)
    for i in range(n - 1):
        # with replicas, train_d leaves its gradient exchange in flight: the D update is applied by the next half
        # step right before it first needs the D parameters (after train_g_d's generator forward)
        kw = {}
        if i == n - 2 and grad_sync is None and gan_model is xmc_gan:
            kw["next_g_batch"] = parts[-1]           # its generator forward runs beside this half step's backward
            kw["next_g_rng"] = rngs[-1]
        state = gan_model.train_d(rngs[i], state, parts[i], generator, discriminator, config, grad_sync=grad_sync,
                                  defer_update=grad_sync is not None, **kw)
    return gan_model.train_g_d(rngs[-1], state, parts[-1], generator, discriminator, config, additional_data or {},
                               grad_sync=grad_sync)


# hipStreamCaptureModeThreadLocal: only the capturing thread is held to the capture rules.  Under the default
# ("global") mode ANY thread's hipEventQuery aborts the capture -- and ProcessGroupNCCL's watchdog thread polls the
# end events of the eager collectives issued just before (every 100 ms, until it has seen them complete): a rare
# "operation not permitted when stream is capturing" + SIGABRT under torchrun (seen once in ~15 runs, round 3).
CAPTURE_ERROR_MODE = "thread_local"
WATCHDOG_DRAIN_S = 0.35


class GraphedTrainStep:
    """``train_step`` captured ONCE into a hipGraph and replayed.

    One eager ``train_step`` issues ~700 kernel launches through Python + ctypes (17-25 ms of host time); the
    captured graph is one ``hipGraphLaunch``.  What makes the step replayable:

    * every buffer a kernel touches is caller-owned (torch's caching allocator serves the capture from a private
      pool: the tape, workspaces and scratch of the step keep fixed addresses);
    * the batch lives in static tensors (``load_batch`` copies a new batch into them);
    * the Adam step counters live in device memory (``ParamArena.step_state``, xmc_adam_ema_dev);
    * parameters / moments / EMA are updated in place in their arenas, and the per-step state the reference
      returns as new pytrees -- G's BatchNorm running statistics, D's spectral-norm ``u0`` -- is copied back into
      the persistent flat buffers (``FlatTree``) at the end of the graph.

    Call the eager ``train_step`` at least once before constructing this (lazy per-device setup in the library,
    RCCL communicator creation), then ``state, metrics = graphed(state, batch)``.  ``accumulator`` (a ``MetricAccumulator``):
    its launch is captured behind the step, so every replay also adds the step's metrics to the running sums.  ``state`` must be the object
    this instance returned last (or was built from): the graph owns the addresses of its tensors.
    """

    def __init__(self, state, batch, gan_model=xmc_gan, generator=None, discriminator=None, config=None,
                 additional_data=None, grad_sync=None, accumulator=None):
        g, d = generator(train=True), discriminator(train=True)
        ops = g.ops
        dev = ops.device
        self.config = config
        if "z" not in batch:
            raise ValueError("GraphedTrainStep needs the noise in the batch (key 'z', coco_dataset.py:165-166): a "
                             "host-seeded draw inside train_d / train_g_d cannot be replayed by a captured graph")
        self.static_batch = {k: torch.as_tensor(v).to(dev).clone() for k, v in batch.items()}
        # config.diff_augment: a capture cannot read the plan back, so its host copy is made here.  It is the CAPTURE-TIME plan:
        # the library validates it once, while capturing; a replayed plan reaches the kernels through the static tensor only, and
        # their clamps and bounds checks are what protects a replay
        aug_host = torch.from_numpy(xmc_gan.plan_host_of(batch["d_aug"]).copy()).pin_memory() if "d_aug" in batch else None
        state = xmc_gan._flush(state)
        bs = g.flat_batch_stats(state.g_optimizer.target, state.generator_state["batch_stats"])
        sn = d.flat_sn_stats(state.d_optimizer.target, state.discriminator_state["spectral_norm_stats"])
        state = state.replace(generator_state={"batch_stats": bs}, discriminator_state={"spectral_norm_stats": sn})
        ga, da = state.g_optimizer.arena, state.d_optimizer.arena
        before = (ga.opt_step, da.opt_step, int(state.step))
        if additional_data and "image_model" in additional_data:
            additional_data["image_model"].bind(ops)     # the frozen ResNet-50's weights go to HBM before the capture
        torch.cuda.synchronize(dev)
        if grad_sync is not None:
            # ProcessGroupNCCL's watchdog keeps every eager collective in its list until it has SEEN it complete (it looks every
            # ~100 ms).  If the capture puts RCCL's stream into capture mode while such an entry is still there, the watchdog's
            # hipEventQuery on that (eagerly recorded) end event fails with "operation not permitted on an event last recorded
            # in a capturing stream" and the process aborts -- seen once in round 4 (profiles/r04: the D-exchange-in-one-piece
            # run).  All collectives are complete here (synchronize above): give the watchdog three of its periods to retire them.
            time.sleep(WATCHDOG_DRAIN_S)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode=CAPTURE_ERROR_MODE):
            new_state, metrics = train_step(0, state, self.static_batch, gan_model, generator, discriminator, config,
                                            additional_data or {}, grad_sync=grad_sync,
                                            **({"d_aug_host": aug_host} if aug_host is not None else {}))
            new_state = xmc_gan._flush(new_state)
            guard = getattr(new_state, "guard", None)
            if guard is None:
                bs.flat.copy_(new_state.generator_state["batch_stats"].flat)
                sn.flat.copy_(new_state.discriminator_state["spectral_norm_stats"].flat)
            else:
                # config.skip_nonfinite_updates: every half step committed its statistics and u0 into the persistent flat buffers
                # itself (xmc_commit_if, under its verdict: the unconditional copies would undo a skip) -- nothing is left to copy
                # (``commit`` returns at once for a buffer onto itself)
                guard.commit(ops, bs.flat, new_state.generator_state["batch_stats"].flat)
                guard.commit(ops, sn.flat, new_state.discriminator_state["spectral_norm_stats"].flat)
            if accumulator is not None:                  # the step's metrics are summed on the device: still one graph launch
                accumulator.add(metrics, verdict=guard.verdict if guard is not None else None)
        # capture executed nothing: undo the host-side mirrors the Python code advanced, keep what a replay must add
        self._d_steps, self._g_steps = da.opt_step - before[1], ga.opt_step - before[0]
        self._steps = int(new_state.step) - before[2]
        ga._opt_step, da._opt_step = before[0], before[1]
        ga.version += 1                                  # prepared-weight caches point into the graph's pool:
        da.version += 1                                  # any eager call after this must re-prepare
        self.state, self.metrics = state, metrics
        # ops.fuse_prep: the captured forward passes trust the prepared copies the previous step's optimiser kernel left in the
        # networks' persistent buffers; parameters changed behind the graph's back (load_flax_params, an eager step) are
        # detected by the arenas' version counters and re-prepared eagerly before the replay
        self._nets, self._versions = (g, d), (ga.version, da.version)
        # the graph reads buffers only ``additional_data`` owns (the frozen ResNet-50's weights and persistent tensors, the
        # statistics' vectors): they must live as long as the graph does
        self._additional_data = additional_data

    def load_batch(self, batch):
        for k, dst in self.static_batch.items():
            src = torch.as_tensor(batch[k])
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src, non_blocking=True)

    def __call__(self, state=None, batch=None):
        """Replay one step.  ``batch`` (optional) is copied into the static input tensors first.
        -> (state, metrics): metrics are the graph's static output tensors (read them before the next replay)."""
        if state is not None and state is not self.state:
            raise ValueError("GraphedTrainStep replays on the state it returned last (the graph owns its buffers)")
        if batch is not None:
            self.load_batch(batch)
        st = self.state
        if (st.g_optimizer.arena.version, st.d_optimizer.arena.version) != self._versions:
            g, d = self._nets
            if hasattr(g, "refresh_prepared"):
                g.refresh_prepared(st.g_optimizer.target)
                d.refresh_prepared(st.d_optimizer.target, st.discriminator_state["spectral_norm_stats"])
        self.graph.replay()
        st.g_optimizer.arena.note_steps(self._g_steps)
        st.d_optimizer.arena.note_steps(self._d_steps)
        st.g_optimizer.arena.version += 1
        st.d_optimizer.arena.version += 1
        self._versions = (st.g_optimizer.arena.version, st.d_optimizer.arena.version)
        st.step += self._steps
        return st, self.metrics


def eval_step(rng, state, batch, generator, config):
    """Generator-only evaluation (train_utils.py:245-281, eval_metrics.py:90-124): images from the
    current and from the EMA parameters with running BatchNorm statistics; z ~ N(0, 1) from ``rng``
    unless the batch carries one."""
    if not config.get("ema", True) and int(state.step) > 0:
        import warnings
        warnings.warn("config.ema is False (the build-side switch of the C1 / C3 benchmark configs): the EMA parameters "
                      "were not updated by train_g_d and still hold their initial values", stacklevel=2)
    g = generator(train=False)
    cond = {k: batch[k] for k in ("sentence_embedding", "embedding", "max_len")}
    b = torch.as_tensor(batch["sentence_embedding"]).shape[0]
    if "z" in batch:
        z = batch["z"]
    else:
        gen = torch.Generator().manual_seed(int(rng))
        z = torch.randn((b, config.z_dim), generator=gen)
    variables = {"params": state.g_optimizer.target, **state.generator_state}
    image = g.apply(variables, (cond, z), mutable=False)
    ema_variables = {"params": state.ema_params, **state.generator_state}
    ema_image = g.apply(ema_variables, (cond, z), mutable=False)
    return image, ema_image


def generate_from_captions(rng, state, captions, generator, config, text_encoder):
    """Text in, images out: ``captions`` (a list of strings) -> ``(image, ema_image)`` of ``eval_step``.  ``text_encoder``: a
    ``utils.bert_utils.TextEncoder``.  The ``cond`` dict is built as ``coco_dataset.preprocess`` builds it (coco_dataset.py:127-167):
    float32 ``embedding`` (N, T, 768) and ``sentence_embedding`` (N, 768), ``max_len`` as (N, 1) float.  T is
    ``config.max_text_length`` if set, else 64 for ``coco_version == "ln"``, else 17."""
    # the caption length the model was trained at: Localized Narratives (coco_version = "ln") pads to 64 tokens, COCO to 17
    default_t = syn.LN_MAX_WORDS if config.get("coco_version", "2014") == "ln" else syn.MAX_WORDS
    t = int(config.get("max_text_length", None) or default_t)
    embedding, sentence, max_len = text_encoder.get_bert_for_captions(list(captions), t)
    batch = {"embedding": torch.as_tensor(embedding, dtype=torch.float32),
             "sentence_embedding": torch.as_tensor(sentence, dtype=torch.float32),
             "max_len": torch.as_tensor(max_len.astype("float32"))[:, None]}
    return eval_step(rng, state, batch, generator, config)


def generate_sample(rng, state, generator, config, cond=None, world_size=1):
    """Single-device sampling with a fresh ``z`` (reference train_utils.py:196-242) -> ``{"generated_image", "ema_generated_image"}``,
    each a ``make_grid`` of ``config.show_num`` images with the writer's leading [None] axis.  ``sample_size`` =
    ``config.batch_size // world_size`` (the reference divides by ``jax.device_count()``).

    The reference conditions on ``dict(sentence_embedding=one_hot(label, config.num_classes))`` -- a leftover of a class-conditional
    model: ``xmc_net.Generator`` reads ``embedding`` and ``max_len`` too (xmc_net.py:170-172), so the reference call raises
    ``KeyError('embedding')`` for every XMC config.  Called the same way (``cond=None``) this raises the same KeyError; with
    ``cond`` = a caption dict (``sentence_embedding``, ``embedding``, ``max_len``; leading dim >= sample_size) it samples."""
    from .utils import image_utils
    sample_size = config.batch_size // max(int(world_size), 1)
    gen = torch.Generator().manual_seed(int(rng))
    z = torch.randn((sample_size, config.z_dim), generator=gen)
    if cond is None:
        label = torch.randint(0, 1000, (sample_size,), generator=gen)
        cond = dict(sentence_embedding=torch.nn.functional.one_hot(label, config.get("num_classes", 1000)).float())
    missing = [k for k in ("embedding", "max_len") if k not in cond]
    if missing:
        raise KeyError(missing[0])
    cond = {k: torch.as_tensor(cond[k])[:sample_size] for k in ("sentence_embedding", "embedding", "max_len")}
    g = generator(train=False)
    image = g.apply({"params": state.g_optimizer.target, **state.generator_state}, (cond, z), mutable=False)
    ema_image = g.apply({"params": state.ema_params, **state.generator_state}, (cond, z), mutable=False)
    show = config.get("show_num", 64)
    return dict(generated_image=image_utils.make_grid(image.float(), show)[None],
                ema_generated_image=image_utils.make_grid(ema_image.float(), show)[None])


def generate_batch(rng, state, batch, generator, config, collect_all=False, group=None):
    """Sampling for visualisation / evaluation (reference train_utils.py:245-309): images from
    the current and from the EMA generator parameters (``train=False``: running BatchNorm statistics) and the
    originals, each as a ``make_grid`` of ``config.show_num`` float32 images.  ``collect_all`` concatenates the
    replicas' images first (``lax.all_gather`` of the reference -> ``torch.distributed.all_gather``)."""
    from .utils import image_utils
    image, ema_image = eval_step(rng, state, {k: v for k, v in batch.items() if k != "z"}, generator, config)
    ori = torch.as_tensor(batch["image"]).to(image.device)
    outs = [image.float(), ema_image.float(), ori.float()]
    if collect_all and torch.distributed.is_available() and torch.distributed.is_initialized():
        world = torch.distributed.get_world_size(group)
        gathered = []
        for t in outs:
            parts = [torch.empty_like(t) for _ in range(world)]
            torch.distributed.all_gather(parts, t.contiguous(), group=group)
            gathered.append(torch.cat(parts, dim=0))
        outs = gathered
    show = config.get("show_num", 64)
    # key names and the leading [None] axis of the reference's summary dict (train_utils.py:299-309)
    return {"generated_image_batch": image_utils.make_grid(outs[0], show)[None],
            "ema_generated_image_batch": image_utils.make_grid(outs[1], show)[None],
            "ori_image_batch": image_utils.make_grid(outs[2], show)[None]}


# ==================================================================================== the training and evaluation loops
# (reference train_utils.py:312-514.  DESIGN.md section 9e lists every departure.)
EVAL_KEYS = ("fid", "fid_std", "inception_score", "inception_score_std", "ema_fid", "ema_fid_std", "ema_inception_score",
             "ema_inception_score_std")          # the order ``EvalMetric.calculate_inception_fid`` returns them in
MAX_TO_KEEP = 5


def fold_in(seed, *data):
    """``jax.random.fold_in`` stand-in on integer seeds: a pure function of ``(seed, *data)``, 48 bits wide so that
    ``train_step``'s ``rng * d_step_per_g_step + i`` stays a valid ``torch.Generator`` seed."""
    import numpy as np
    state = np.random.SeedSequence([int(seed) & 0xFFFFFFFFFFFFFFFF] + [int(d) for d in data])
    return int(state.generate_state(1, np.uint64)[0] >> np.uint64(16))


def rng_streams(seed):
    """The independent streams both loops derive from ``config.seed`` (the reference splits one PRNGKey, :323-357,414): ``data``
    (the rank is folded in by ``create_datasets``), ``model`` (``create_train_state``), ``train`` (folded with the step for the
    eager ``train_step``), ``sample_batch`` (z of the sample grids, folded with the step), ``eval`` (``test``'s z)."""
    return {name: fold_in(seed, i) for i, name in enumerate(("data", "model", "train", "sample_batch", "eval"))}


def default_datasets(config, data_rng, start_step, rank, world, device):
    """The ``datasets`` hook of ``train`` / ``test`` over the real pipeline.  A fresh run (``start_step`` 1) seeds the pipeline
    with ``data_rng``; a run resumed at step ``s`` seeds it with ``fold_in(data_rng, s)`` -- the pipeline's position cannot be
    checkpointed as the reference's tf.data iterator is, so a resumed run draws a new order instead of replaying the batches
    the first run began with."""
    from .libml import input_pipeline
    seed = data_rng if start_step <= 1 else fold_in(data_rng, start_step)
    return input_pipeline.create_datasets(config, seed, rank=rank, world=world, device=device)


def resolve_num_train_steps(config, num_train_examples, local_devices=1, test_mode=False):
    """``config.num_train_steps``, or for -1 the reference's rule (:339-352): ``mscoco`` trains ``num_epochs`` epochs of
    ``num_train_examples // (local devices * d_step_per_g_step)`` steps; any other dataset trains its cardinality (here: the
    hook's ``num_train_examples``), or one step in ``test_mode``."""
    n = int(config.num_train_steps)
    if n != -1:
        return n
    if config.get("dataset", "mscoco") == "mscoco":
        steps_per_epoch = int(num_train_examples) // (int(local_devices) * int(config.d_step_per_g_step))
        return steps_per_epoch * int(config.num_epochs)
    return 1 if test_mode else int(num_train_examples)


class MetricAccumulator:
    """Float64 running sums of a step's scalar metrics, the number of steps added and the first step that held a non-finite
    value, all in device memory: on ``HipOps`` one ``xmc_metrics_accum`` launch per ``add`` (capturable: ``GraphedTrainStep``
    records it behind the step, so a replayed step needs no host read); on an operator table without ``metrics_accum`` the same
    arithmetic in torch.  ``read`` is the only host synchronisation."""

    def __init__(self, keys, ops=None, device=None):
        self.keys = tuple(keys)
        if not 1 <= len(self.keys) <= 8:
            raise ValueError("MetricAccumulator holds 1 to 8 metrics")
        self.ops = ops if hasattr(ops, "metrics_accum") else None
        device = device if device is not None else (ops.device if ops is not None else torch.device("cpu"))
        self.sums = torch.zeros((len(self.keys),), dtype=torch.float64, device=device)
        self.info = torch.zeros((2,), dtype=torch.int32, device=device)         # [calls, 1-based first call with a non-finite value]

    def add(self, metrics, verdict=None):
        """``verdict`` (config.skip_nonfinite_updates: the int32[4] of the train_g_d that produced ``metrics``, device memory): a
        skipped half step adds nothing and is not counted -- decided on the device (``xmc_metrics_accum_if``)"""
        vals = [torch.as_tensor(metrics[k]).detach().reshape(-1) for k in self.keys]
        if self.ops is not None:
            vals = [v if v.dtype == torch.float32 else v.float() for v in vals]
            if verdict is not None:
                self.ops.metrics_accum_if(vals, self.sums, self.info, verdict)
            else:
                self.ops.metrics_accum(vals, self.sums, self.info)
            return
        if verdict is not None and int(verdict[0]) != 0:
            return
        v = torch.cat([t.to(self.sums.device, torch.float32) for t in vals])
        self.sums += v.double()
        self.info[0] += 1
        if not bool(torch.isfinite(v).all()) and int(self.info[1]) == 0:
            self.info[1] = self.info[0]

    def read(self):
        """-> ({key: float64 sum}, number of ``add`` calls, first call with a non-finite value or 0)"""
        sums = self.sums.cpu().tolist()
        count, first_bad = self.info.cpu().tolist()
        return dict(zip(self.keys, sums)), count, first_bad

    def reset(self):
        self.sums.zero_()
        self.info.zero_()


class CheckpointRotation:
    """``ckpt-<n>.flax`` files of one directory: ``n`` is the save ordinal, continuing from the highest one present (the reference's
    checkpoint library numbers its saves, not the steps); the newest ``max_to_keep`` are kept.  A file appears under its final
    name only when it is complete (written under a temporary name, then renamed)."""

    def __init__(self, directory, max_to_keep=MAX_TO_KEEP):
        self.directory, self.max_to_keep = directory, int(max_to_keep)

    def all(self):
        from .utils import task_manager
        return task_manager.list_checkpoints(self.directory)

    def latest(self):
        found = self.all()
        return found[-1] if found else None

    def save(self, state):
        import os
        from .utils import checkpoint, task_manager
        os.makedirs(self.directory, exist_ok=True)
        latest = self.latest()
        n = task_manager.checkpoint_number(latest) + 1 if latest else 1
        path = os.path.join(self.directory, f"ckpt-{n}.flax")
        tmp = os.path.join(self.directory, f".ckpt-{n}.flax.tmp{os.getpid()}")
        checkpoint.save(tmp, state)
        os.replace(tmp, path)
        for old in self.all()[:-self.max_to_keep]:
            os.remove(old)
        return path


class JsonlWriter:
    """Scalars as one JSON object per line (``{"step": s, name: value, ...}``), appended to ``path``."""

    def __init__(self, path):
        self.path = path

    def write_scalars(self, step, scalars):
        import json
        with open(self.path, "a") as f:
            f.write(json.dumps({"step": int(step), **{k: float(v) for k, v in scalars.items()}}) + "\n")


def write_layer_stats(path, step, window):
    """One line per scalar-writing boundary: ``{"step": s, "count": steps in the window, "leaves": {"d/<path>" | "g/<path>":
    {"grad_norm_rms", "param_norm_rms", "nonfinite"}}}`` from ``TrainStatistics.read()`` -- per physical tensor of the arenas the
    RMS over the window of the per-step gradient norm, of the parameter norm, and the non-finite gradient elements seen."""
    import json
    n = max(window["count"], 1)
    leaves = {name: {"grad_norm_rms": (gsq / n) ** 0.5, "param_norm_rms": (psq / n) ** 0.5, "nonfinite": int(bad)}
              for name, (gsq, psq, bad) in window["leaves"].items()}
    with open(path, "a") as f:
        f.write(json.dumps({"step": int(step), "count": int(window["count"]), "leaves": leaves}) + "\n")


def write_image_grids(directory, step, image_dict):
    """Each ``(1, H, W, 3)`` float grid of ``generate_batch`` (values in [0, 1]) as ``<directory>/<name>_<step>.png``"""
    import os
    from .libml import png
    os.makedirs(directory, exist_ok=True)
    paths = {}
    for name, grid in image_dict.items():
        px = (grid[0].detach().float().clamp(0, 1) * 255.0).round().to(torch.uint8).cpu().numpy()
        paths[name] = os.path.join(directory, f"{name}_{int(step):08d}.png")
        tmp = paths[name] + ".tmp"
        with open(tmp, "wb") as f:
            f.write(png.encode_rgb(px))
        os.replace(tmp, paths[name])
    return paths


def _rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size(), True
    return 0, 1, False


def _array_fields(batch):
    """the tensor fields of a pipeline batch (``return_text`` / ``return_filename`` add lists of bytes the step does not read)"""
    import numpy as np
    return {k: torch.as_tensor(v) for k, v in batch.items() if isinstance(v, (torch.Tensor, np.ndarray))}


def optimizer_rates(state, config):
    """With a schedule (libml/opt_schedule.py): the learning rates and the EMA decay of the optimisers' last updates ->
    ``{"opt/g_lr", "opt/d_lr", "opt/ema_decay"}``.  Read from slots 4 and 5 of the arenas' ``step_state``, where the scheduled
    advance kernel left them (a host synchronisation: ``train`` calls it where it reads the metric sums anyway); on an operator
    table without a device counter, the specification at the host's t.  Before the first update every value is 0."""
    from .libml import opt_schedule
    out = {}
    for role, opt in (("g", state.g_optimizer), ("d", state.d_optimizer)):
        a = opt.arena
        if a.step_state is not None:
            now = opt_schedule.read_slots(a.step_state)
            lr, decay = now["lr"], now["ema_decay"]
        elif a.opt_step < 1:
            lr = decay = 0.0
        else:
            ema = role == "g" and config.get("ema", True)
            s = opt_schedule.for_optimizer(config, role, config.g_lr if role == "g" else config.d_lr, config.polyak_decay if ema else 0.0)
            lr, decay = (float(x) for x in opt_schedule.evaluate(s, a.opt_step)[:2])
        out[f"opt/{role}_lr"] = lr
        if role == "g":
            out["opt/ema_decay"] = decay
    return out


def check_replica_drift(states, grad_sync):
    """The tripwire of DESIGN.md 9f.3: ``states`` maps a controller's name to its small device state (float64[8] / int32[4]; None =
    the switch is off), which every replica must hold BIT FOR BIT -- rank 0's checkpoint is then everybody's.  The states are
    all-gathered and compared on the host (``train`` reads them at a checkpoint boundary anyway); RuntimeError names the
    controller and the first rank that differs from rank 0."""
    import torch.distributed as dist
    for name, t in sorted(states.items()):
        if t is None:
            continue
        bits = t.detach().contiguous().view(torch.int32).reshape(-1)
        out = torch.empty((grad_sync.world, bits.numel()), dtype=torch.int32, device=bits.device)
        dist.all_gather_into_tensor(out.view(-1), bits, group=grad_sync.group)
        out = out.cpu()
        for r in range(1, grad_sync.world):
            if not torch.equal(out[r], out[0]):
                raise RuntimeError(f"train: the {name} controller's state on rank {r} differs from rank 0's: the replicas have "
                                   f"drifted apart, and a checkpoint would hold rank 0's state alone (as int32 words: rank 0 "
                                   f"{out[0].tolist()}, rank {r} {out[r].tolist()})")


def train(config, workdir, test_mode=False, *, datasets=None):
    """The training loop (reference train_utils.py:312-461).  Resumes from the newest checkpoint of ``workdir/checkpoints-0``;
    every ``eval_every_steps`` (and on the last step) the averaged train metrics go to ``workdir/metrics.jsonl`` and three sample
    grids to ``workdir/images/``; every ``checkpoint_every_steps`` (and on the last step) a checkpoint is written; ``TRAIN_DONE``
    marks the end.  ``datasets``: ``(config, data_rng, start_step, rank, world, device) -> (train_iter, eval_iter,
    num_train_examples)`` (default: ``default_datasets``).  On ``HipOps`` the first step of the call runs eagerly, the others
    replay one captured graph with the metric accumulator inside; on an injected operator table every step runs eagerly.
    With ``torch.distributed`` initialised the gradients are exchanged through ``dp.GradSync`` and rank 0 alone writes files.
    Returns the final ``TrainState``."""
    import os
    from .utils import checkpoint, task_manager
    rank, world, distributed = _rank_world()
    writes = rank == 0
    if config.get("model_name", "xmc") != "xmc":
        raise NotImplementedError(f"{config.model_name} was not Implemented!")
    gan_model = xmc_gan
    if writes:
        os.makedirs(workdir, exist_ok=True)
    streams = rng_streams(config.seed)
    additional_data = gan_model.create_additional_data(config)
    generator, discriminator, state = create_train_state(config, streams["model"])
    ops = generator.ops
    manager = task_manager.TaskManagerWithCsvResults(os.path.join(workdir, "checkpoints"))
    rotation = CheckpointRotation(manager.model_dir)
    latest = rotation.latest()
    if latest is not None:
        state = checkpoint.restore(latest, state)
    initial_step = int(state.step) + 1
    device = ops.device if ops.device.type == "cuda" else None
    train_iter, _eval_iter, num_train_examples = (datasets or default_datasets)(config, streams["data"], initial_step, rank, world,
                                                                                 device)
    num_train_steps = resolve_num_train_steps(config, num_train_examples, int(os.environ.get("LOCAL_WORLD_SIZE", world)), test_mode)
    from .libml import opt_schedule
    config = opt_schedule.resolve(config, num_train_steps)     # a decaying schedule without lr_decay_end_step ends with the run
    scheduled = opt_schedule.enabled(config)
    grad_sync = None
    if distributed:
        from .dp import GradSync
        bn_groups = generator(train=True).bn_groups
        # cross-replica BatchNorm groups issue collectives from inside the generator's passes: only the exclusive schedule
        # keeps the gradient exchange out of their way (dp.check_schedule)
        # ... and config.ada_target, config.lecam_weight and config.skip_nonfinite_updates are decided from rows that the replicas
        # all-gather on the gradient communicator (GradSync.gather_rows): the exclusive schedule too
        from .libml import ada as _ada, lecam as _lecam, nonfinite_guard as _guard
        shared = _ada.enabled(config) or _lecam.enabled(config) or _guard.enabled(config)
        grad_sync = GradSync(schedule="exclusive", bn_groups=bn_groups) if (bn_groups is not None or shared) else GradSync()
    if writes and initial_step == 1:                 # the reference's writer.write_hparams (:402-403)
        import json
        with open(os.path.join(workdir, "config.json"), "w") as f:
            json.dump(dict(config), f, indent=1, sort_keys=True, default=str)
    use_graph = ops.device.type == "cuda" and xmc_net._OPS_FACTORY is None
    accumulator = MetricAccumulator(xmc_gan.metric_keys(config), ops)
    writer = JsonlWriter(os.path.join(workdir, "metrics.jsonl"))
    statistics = additional_data.get("statistics")   # config.train_statistics: filled by train_g_d, read at the boundaries below
    graphed, window_start = None, initial_step
    n_split = config.d_step_per_g_step
    from .libml import ada as ada_lib
    from .libml import diff_augment
    aug_policy = config.get("diff_augment", "")      # differentiable augmentation of D's inputs: a plan per step, like z
    ada = state.ada if ada_lib.enabled(config) else None       # config.ada_target: p is decided on the device
    from .libml import lecam as lecam_lib
    lecam = state.lecam if lecam_lib.enabled(config) and gan_model is xmc_gan else None      # config.lecam_weight: the anchors
    clip_guidance = additional_data.get("clip_guidance") if gan_model is xmc_gan else None      # config.clip_guidance_weight > 0
    from .libml import nonfinite_guard
    guard = state.guard if nonfinite_guard.enabled(config) else None      # config.skip_nonfinite_updates: the skip counters
    skipped_before = guard.read()["skipped"] if guard is not None else 0
    for step in range(initial_step, num_train_steps + 1):
        is_last_step = step == num_train_steps
        item = next(train_iter)
        batch = {k: v.to(ops.device) for k, v in _array_fields(item).items()}
        if clip_guidance is not None:
            # the frozen CLIP text tower on this step's captions: eagerly, on the step's stream, BETWEEN graph launches (the
            # token ids are validated on the host) -- a device tensor that load_batch copies into the graph's static batch
            from .utils.eval_metrics import _captions
            if "text" not in item:
                raise ValueError('clip_guidance_weight > 0 needs the captions\' text in every training batch (batch["text"]: '
                                 "COCODataset(return_caption_text=True), which create_datasets sets on the training stream)")
            batch["clip_text"] = clip_guidance.embed_text(ops, _captions(item))
        if aug_policy:
            # a pure function of (seed, step, rank): a resumed run draws what the uninterrupted one did.  Left on the host -- the
            # eager step validates it there, GraphedTrainStep.load_batch copies it into the graph's static tensor
            rows, h, w = batch["image"].shape[:3]
            batch["d_aug"] = torch.from_numpy(diff_augment.draw_plan(fold_in(streams["train"], step), step, rank, rows, h, w,
                                                                     aug_policy))
            if ada is not None:                      # ... and the uniforms its parts are gated with, a stream of their own
                batch["d_aug_u"] = torch.from_numpy(ada_lib.draw_gates(fold_in(streams["train"], step), step, rank, rows))
        if graphed is None:
            state, metrics = train_step(fold_in(streams["train"], step), state, batch, gan_model, generator, discriminator, config,
                                        additional_data, grad_sync=grad_sync)
            accumulator.add(metrics, verdict=guard.verdict if guard is not None else None)
            if use_graph and not is_last_step:
                graphed = GraphedTrainStep(state, batch, gan_model, generator, discriminator, config, additional_data,
                                           grad_sync=grad_sync, accumulator=accumulator)
                state = graphed.state
        else:
            state, metrics = graphed(state, batch)
        write_scalars = step % config.eval_every_steps == 0 or is_last_step
        write_checkpoint = step % config.checkpoint_every_steps == 0 or is_last_step
        if not (write_scalars or write_checkpoint):
            continue
        sums, count, first_bad = accumulator.read()
        if first_bad:
            where = ""
            if statistics is not None:
                bad = statistics.read()["first_bad"]
                where = (f"; the first gradient that held a non-finite value was {bad[1]} at step {window_start + bad[0] - 1}"
                         if bad else "; no gradient held a non-finite value")
            raise FloatingPointError(f"train: a training metric was not finite at step {window_start + first_bad - 1}; "
                                     f"no checkpoint of that state is written (the newest one is {rotation.latest()}){where}")
        skips = guard.read() if guard is not None else None       # read together with the accumulator: one synchronisation
        if skips is not None and skips["longest"] >= nonfinite_guard.max_consecutive(config):
            where = ""
            if statistics is not None:
                bad = statistics.read()["first_bad"]
                where = (f"; the first gradient that held a non-finite value was {bad[1]} at step {window_start + bad[0] - 1}"
                         if bad else "; no gradient held a non-finite value")
            raise FloatingPointError(f"train: {skips['longest']} consecutive half steps were skipped for non-finite values "
                                     f"(config.nonfinite_max_consecutive = {nonfinite_guard.max_consecutive(config)}) by step {step}: "
                                     f"the parameters or the data are bad and skipping cannot help; no checkpoint of that state is "
                                     f"written (the newest one is {rotation.latest()}){where}")
        ada_now = ada.read() if ada is not None else None         # (with the accumulator too: the stream is already drained)
        lecam_now = lecam.read() if lecam is not None else None   # (likewise)
        rates_now = optimizer_rates(state, config) if scheduled else None      # (likewise: the two step states)
        state = xmc_gan._flush(state)
        if write_scalars:
            # (a window whose every step was skipped has no metric to average: NaN, as 0 / 0 says)
            scalars = {k: sums[k] / count if count else float("nan") for k in accumulator.keys}
            if skips is not None:
                scalars["guard/skipped_half_steps"] = skips["skipped"] - skipped_before
                scalars["guard/longest_run"] = skips["longest"]
                skipped_before = skips["skipped"]
                guard.reset_longest()
            if ada_now is not None:
                scalars.update({"ada/p": ada_now["p"], "ada/r_t": ada_now["r_t"], "ada/adjustments": ada_now["adjustments"]})
            if lecam_now is not None:
                scalars.update({"lecam/anchor_real": lecam_now["anchor_real"], "lecam/anchor_fake": lecam_now["anchor_fake"],
                                "lecam/updates": lecam_now["updates"]})
            if rates_now is not None:                # the rates of the LAST update of the window, as the kernels read them
                scalars.update(rates_now)
            if statistics is not None:               # this replica's statistics (not averaged over replicas): window means
                window = statistics.read()
                if writes:
                    scalars.update({f"stats/{k}": v / max(window["count"], 1) for k, v in window["sums"].items()})
                    write_layer_stats(os.path.join(workdir, "layer_stats.jsonl"), step, window)
                statistics.reset()
            if writes:
                writer.write_scalars(step, scalars)
            accumulator.reset()
            window_start = step + 1
            if writes:
                visualize = split_input_dict(batch, n_split)[0]
                grids = generate_batch(fold_in(streams["sample_batch"], step), state, visualize, generator, config)
                write_image_grids(os.path.join(workdir, "images"), step, grids)
        if write_checkpoint and grad_sync is not None:
            check_replica_drift({"ada": ada.state if ada is not None else None, "lecam": lecam.state if lecam is not None else None,
                                 "guard": guard.counters if guard is not None else None}, grad_sync)
        if write_checkpoint and writes:
            if guard is not None:                    # Adam's t on the host = the number of APPLIED updates (the device's counter)
                state.g_optimizer.arena.sync_opt_step()
                state.d_optimizer.arena.sync_opt_step()
            rotation.save(state)
    if writes:
        manager.mark_training_done()
    return state


def test(config, workdir, *, datasets=None, inception_ckpt_path=None, inception=None, timeout=24 * 3600, task_manager_kw=None,
         clip=None):
    """The evaluation loop (reference train_utils.py:464-514): FID and Inception Score, from the current and from the EMA
    parameters, of every checkpoint of ``workdir/checkpoints-0`` that has no row in its ``scores.csv`` yet; waits for new
    checkpoints until ``timeout`` seconds pass without one or ``TRAIN_DONE`` appears.  The eight values go as ``eval/<name>`` to
    ``scores.csv`` and to ``workdir/metrics.jsonl``; with ``config.eval_extra_metrics`` (``"kid"``, ``"precision_recall"``, ``"clip"``) so do the
    values ``EvalMetric.calculate_metrics`` adds.  A ``scores.csv`` that was started with another set of columns raises ValueError
    before anything is evaluated.  ``inception`` / ``inception_ckpt_path``: see ``EvalMetric`` (which is built
    when the first checkpoint is found); ``clip``: its injected CLIP scorer (``"clip"`` only).  Returns the number of checkpoints
    evaluated."""
    import os
    import torch.distributed as dist
    from .utils import checkpoint, eval_metrics, task_manager
    rank, world, distributed = _rank_world()
    streams = rng_streams(config.seed)
    generator, _, state = create_train_state(config, streams["model"])
    ops = generator.ops
    device = ops.device if ops.device.type == "cuda" else None
    _, eval_iter, _ = (datasets or default_datasets)(config, streams["data"], 1, rank, world, device)
    manager = task_manager.TaskManagerWithCsvResults(os.path.join(workdir, "checkpoints"), **(task_manager_kw or {}))
    writer = JsonlWriter(os.path.join(workdir, "metrics.jsonl"))
    extras = tuple(config.get("eval_extra_metrics", ()))
    keys = EVAL_KEYS + eval_metrics.extra_metric_keys(extras)
    if os.path.exists(manager.score_file):        # its header was fixed by the first row: a run with other metrics needs another file
        with open(manager.score_file, newline="") as f:
            have = sorted(c for c in f.readline().rstrip("\r\n").split(",") if c.startswith("eval/"))
        want = sorted(f"eval/{k}" for k in keys)
        if have != want:
            raise ValueError(f"{manager.score_file} has the columns {have}, this evaluation (eval_extra_metrics={extras}) writes "
                             f"{want}: move the file away or evaluate with the metrics it was started with")
    eval_metric, done = None, 0
    for path in manager.unevaluated_checkpoints(timeout=timeout):
        if eval_metric is None:
            eval_metric = eval_metrics.EvalMetric(eval_iter, config, inception_ckpt_path=inception_ckpt_path, inception=inception,
                                                  chunk=int(config.get("eval_chunk", 256)),
                                                  group=dist.group.WORLD if distributed else None, clip=clip)
        state = checkpoint.restore(path, state)
        if extras:
            values = eval_metric.calculate_metrics(generator, state, streams["eval"])
            result = {f"eval/{k}": values[k] for k in keys}
        else:
            values = eval_metric.calculate_inception_fid(generator, state, streams["eval"])
            result = {f"eval/{k}": v for k, v in zip(EVAL_KEYS, values)}
        if rank == 0:
            os.makedirs(workdir, exist_ok=True)
            manager.add_eval_result(path, result, -1)
            writer.write_scalars(int(state.step), result)
        done += 1
    return done
