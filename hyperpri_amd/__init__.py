"""hyperpri_amd -- MI355X-native (gfx950) implementation of the HyperPRI segmentation hot path.

Drop-in ``torch.nn.Module`` replacements for the reference's ``src/Experiments/models.py`` and
``model_parts.py`` whose forward/backward run in hand-written HIP kernels.  See DESIGN.md.
"""
from .cache import (CubeAugment, CubeCache, CubeDeform, deform_entries, elastic_lattice, plan_epoch, plan_epoch_augmented,  # noqa: F401
                    plan_epoch_deformed)
from .cluster import (ClusterSums, SpectralKMeans, assign_reference, cluster_step, cluster_step_reference, kmeans_reference,  # noqa: F401
                      merge_cluster_sums)
from .crf import (CRFLayer, DenseCRF, crf_backward_reference, crf_bound, crf_bruteforce, crf_grad_bound, crf_layer,  # noqa: F401
                  crf_reference, crf_tables, dense_crf)
from .components import (TILE_H, TILE_W, clean_mask, clean_reference, component_table, components_reference,  # noqa: F401
                         label_components)
from .detect import SpectralDetector, detect_reference, whitener_reference  # noqa: F401
from .distance import (boundary_reference, centerline_counts, centerline_from_counts, distance_transform, edt_reference,  # noqa: F401
                       links_reference, root_traits, skeleton_links, skeletonize, soft_skeleton_reference, surface_distances,
                       surface_hist_reference, surface_metrics_from_hist, thin_reference)
from .evaluate import (CLEAN_LOGIT, SplitPrediction, centerline_metrics, clean_prediction, cluster_split, color_classmaps, color_segmaps,  # noqa: F401
                       default_class_palette, detect_split, evaluate_multiclass, object_metrics, predict_split, surface_metrics, test_net, tta_merge,
                       crf_split, enhance_split, fit_crf, gmm_split, refine_split, ridge_split, unmix_split, validate_net, write_segmaps, write_spreadmaps)
from .evaluate import root_traits as split_root_traits  # noqa: F401  (``root_traits`` is the per-tensor call of distance.py)
from .guided import GuidedFilter, guided_bound, guided_bruteforce, guided_filter, guided_reference  # noqa: F401
from .mixture import (GmmOperands, GmmSums, SpectralGMM, gmm_bound, gmm_classes_reference, gmm_operands, gmm_reference,  # noqa: F401
                      gmm_score_reference, gmm_step, gmm_step_reference, gmm_sums_bound, merge_gmm_sums)
from .model_parts import DoubleConv, Down, OutConv, Up, set_precision  # noqa: F401
from .models import (CubeNET, SpectralUNET, UNet, initialize_model, set_parameter_requires_grad,  # noqa: F401
                     translate_load_dir)
from .ridge import RidgeFilter, ridge_bound, ridge_bruteforce, ridge_filter, ridge_reference, ridge_taps  # noqa: F401
from .spectral import (SpectralProjection, SpectralStats, band_statistics, class_spectra, gram_reference, merge_statistics,  # noqa: F401
                       moments_reference, pca_basis, project_reference)
from .tta import TTA, VIEW_NAMES, apply_view, invert_view, tta_merge_reference  # noqa: F401
from .trainer import (BCEWithLogitsLoss, CrossEntropyLoss, DiceBCELoss, DiceLoss, FocalLoss, forward_loss, FusedAdam, FusedSGD,  # noqa: F401
                      LovaszHingeLoss, PRCurve, SegConfusion, SegCounts, SegLoss, SegmentationModel, TverskyLoss, argmax_classes,
                      average_precision, clDiceLoss, load_checkpoint, lovasz_hinge_reference, multiclass_metrics_from_confusion,
                      network_state_dict, ranking_metrics, ranking_reference, soft_skeleton, sort_scores)
from .unmix import (SpectralUnmixer, atgp_reference, extract_endmembers, unmix_bound, unmix_bruteforce, unmix_reference)  # noqa: F401

__version__ = "0.1.0"


def _warn_removed_switches():
    """Environment switches of earlier rounds that no longer exist (folded into HPRI_FUSIONS or dropped): setting one is a silent
    no-op otherwise."""
    import os
    import sys
    gone = ("HPRI_FUSE_BN_REDUCE", "HPRI_FUSE_BN_REDUCE_BF16", "HPRI_CONVT_PLANES", "HPRI_GRAD_BF16_INNER", "HPRI_PLANES_CAT1", "HPRI_YR_BF16",
            "HPRI_WINO4", "HPRI_BUCKET_MB", "HPRI_TAIL_MB")
    hit = [v for v in gone if v in os.environ]
    if hit:
        print("hyperpri_amd: " + ", ".join(hit) + " no longer exist" + ("s" if len(hit) == 1 else "") + ": the per-feature switches are module "
              "attributes of hyperpri_amd.engine under the HPRI_FUSIONS master switch (INTEGRATION.md); GradSync takes bucket_mb / tail_mb "
              "as arguments.", file=sys.stderr)


_warn_removed_switches()
