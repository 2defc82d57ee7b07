"""Hyper-parameters read by the G+D training step.

Mirrors the fields of the reference's ``xmcgan/configs/coco_xmc.py:18-88`` that the hot path
reads ("Config fields read on the hot path").  ``ml_collections`` is not
available in this image, so ``ConfigDict`` is a small attribute-access dict with the same
``config.name`` / ``config["name"]`` surface.
"""
from __future__ import annotations


class ConfigDict(dict):
    """Attribute-access dict (the subset of ml_collections.ConfigDict the path uses)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def copy(self):
        return ConfigDict(self)


def get_config() -> ConfigDict:
    """Default 128 px configuration (reference coco_xmc.py:18-68)."""
    c = ConfigDict()
    c.seed = 42
    # the training / evaluation loops (train_utils.train / test; coco_xmc.py:21-27,30-34,53-54)
    c.num_train_steps = -1          # -1: num_epochs epochs of the training set
    c.log_loss_every_steps = 1000
    c.eval_every_steps = 1000       # train metrics + sample grids are written this often
    c.checkpoint_every_steps = 5000
    c.num_epochs = 500
    c.dataset = "mscoco"
    c.model_name = "xmc"
    c.beta1 = 0.5
    c.beta2 = 0.999
    c.d_lr = 0.0004
    c.g_lr = 0.0001
    c.polyak_decay = 0.999
    c.batch_norm_group_size = -1
    c.dtype = "bfloat16"
    c.image_size = 128
    c.batch_size = 56
    c.eval_batch_size = 7
    c.eval_num = 30000              # images per FID / IS evaluation (coco_xmc.py:23)
    c.eval_avg_num = 3              # evaluation passes averaged (coco_xmc.py:24)
    c.df_dim = 96
    c.gf_dim = 96
    c.z_dim = 128
    c.d_step_per_g_step = 2
    c.g_spectral_norm = False
    c.d_spectral_norm = True
    c.architecture = "xmc_net"
    c.gamma_for_g = 15
    c.word_contrastive = True
    c.sentence_contrastive = True
    c.image_contrastive = True
    # coco_xmc.py:65: the frozen ResNet-50 image-contrastive term.  Its weights come from
    # ``pretrained_model_path`` (the reference's data/resnet_pretrained.npy; a network download -- absent here, the
    # create_additional_data raises FileNotFoundError like the reference; None = explicit random initialisation).
    c.pretrained_image_contrastive = True
    c.pretrained_model_path = "data/resnet_pretrained.npy"
    c.cond_size = 16
    c.show_num = 64                 # images per sampling grid (coco_xmc.py:42)
    # build-side switches (not in the reference)
    c.ema = True
    c.conv_fp8_phase = False        # with conv_fp8: the "out"-form phase launches (conv3x3(upsample2(.))) on the MX-fp8 phase kernel too
    c.conv_fp8_phase_in = False     # with conv_fp8: the "in"-form phase launches (avg_pool2(conv3x3(.))) on the MX-fp8 "in" phase kernel too
    c.device_dataset_cache = False  # decode every record once, keep it in HBM and gather each batch there (libml/device_cache.py)
    # evaluation beyond FID / IS (utils/sample_metrics.py, utils/alignment_metrics.py; EvalMetric.calculate_metrics): names from
    # {"kid", "precision_recall", "clip"}
    c.eval_extra_metrics = ()
    c.kid_subsets = 100             # KID: random subsets per pass ...
    c.kid_subset_size = 1000        # ... of this many rows of each pool
    c.pr_k = 3                      # precision / recall: a row's ball reaches to its pr_k-th nearest other row
    # "clip": CLIPScore and R-precision on a CLIP ViT-B/32 (utils/clip_utils.py); all inert unless "clip" is named
    c.clip_ckpt_path = None         # np.savez of a Hugging Face CLIPModel.state_dict() (None: random weights, meaningless scores)
    c.clip_vocab_path = None        # CLIP's vocab.json ...
    c.clip_merges_path = None       # ... and merges.txt (required with "clip")
    c.clip_fast = False             # bf16 MFMA for the encoder's dense layers
    c.r_precision_candidates = 99   # mismatched captions every image's own caption has to beat
    c.train_statistics = False      # in-graph statistics of train_g_d: head accuracies, D's logits, gradient / parameter norms (train_statistics.py)
    # differentiable augmentation of everything D sees (libml/diff_augment.py; not in the reference): a comma-separated subset of
    # "color", "translation", "cutout"; "" = off, the step is then bit for bit the one without the switch
    c.diff_augment = ""
    return c


def get_test_config() -> ConfigDict:
    """Tiny configuration C0 (reference coco_xmc.py:71-88: dims 16, z 8), per-device B=4."""
    c = get_config()
    c.dtype = "float32"
    c.pretrained_image_contrastive = False      # build-side: the G/D parity tests run without the ResNet-50 term;
    c.batch_size = 4                            # tests/test_resnet.py and tests/test_gpu_resnet.py switch it on
    c.eval_batch_size = 2
    c.eval_num = 2                  # coco_xmc.py:76-77
    c.eval_avg_num = 1
    c.num_train_steps = 2           # coco_xmc.py:78-81
    c.log_loss_every_steps = 1
    c.eval_every_steps = 1
    c.checkpoint_every_steps = 1
    c.num_epochs = 1
    c.show_num = 4                  # coco_xmc.py:85
    c.df_dim = 16
    c.gf_dim = 16
    c.z_dim = 8
    return c


def get_c1_config() -> ConfigDict:
    """BASELINE.json configs[1]: 128 px, gf=df=96, batch 56, bf16, EMA off."""
    c = get_config()
    c.ema = False
    return c


def get_c3_config() -> ConfigDict:
    """BASELINE.json configs[3]: 256 px paper config, per-GPU batch 32."""
    c = get_config()
    c.image_size = 256
    c.batch_size = 32
    c.ema = False
    return c


def get_c4_config() -> ConfigDict:
    """BASELINE.json configs[4]: the 256 px config with fp8 MFMA convolutions -- MX-fp8 operands (e4m3 + e8m0 per 32
    channels) for the 3x3 convolutions' forward and data-gradient passes, float32 accumulation; contrastive losses,
    attention, normalisation and weight gradients as in the bf16 mode (losses in float32)."""
    c = get_c3_config()
    c.conv_fp8 = True
    # scale of an MX block: "next_binade" (default; the OCP conversion, but one binade higher when the block maximum would saturate
    # e4m3) or "ocp_floor" (the OCP MX v1.0 conversion to the letter: clips the largest element of ~1/5 of the blocks by <= 12.5 %)
    c.fp8_scale_rule = "next_binade"
    return c
