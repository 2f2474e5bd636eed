"""hipt_abmil_atec23_amd — MI355X-native (gfx950) implementation of the one data-parallel hot path of
scjjb/HIPT_ABMIL_ATEC23: HIPT_4K feature extraction (ViT-256 -> ViT-4K) and the CLAM_SB / ABMIL
gated-attention pooling, behind the reference's own Python call surface; also the reference's ResNet-50 baseline
extractor (``resnet50_baseline``, the ResNet-ABMIL route).

    from hipt_abmil_atec23_amd import HIPT_4K, CLAM_SB, Attn_Net_Gated
    import hipt_abmil_atec23_amd as amd; amd.install()   # make the reference scripts import these classes

All compute runs in hand-written HIP kernels loaded from ``libhipt_abmil.so`` (C ABI:
``include/hipt_abmil.h``); there is no CPU or eager fallback for inference.
"""
from . import synth  # noqa: F401  (no torch import at package import time)

__all__ = ["HIPT_4K", "CLAM_SB", "CLAM_MB", "Attn_Net", "Attn_Net_Gated", "VisionTransformer",
           "VisionTransformer4K", "vit_small", "vit4k_xs", "install", "build_native"]

_LAZY = {
    "HIPT_4K": ("hipt_4k", "HIPT_4K"),
    "CLAM_SB": ("model_clam", "CLAM_SB"), "CLAM_MB": ("model_clam", "CLAM_MB"),
    "Attn_Net": ("model_clam", "Attn_Net"), "Attn_Net_Gated": ("model_clam", "Attn_Net_Gated"),
    # max-pooling MIL baselines (main.py --model_type mil)
    "MIL_fc": ("model_mil", "MIL_fc"), "MIL_fc_mc": ("model_mil", "MIL_fc_mc"),
    "VisionTransformer": ("vision_transformer", "VisionTransformer"), "vit_small": ("vision_transformer", "vit_small"),
    "VisionTransformer4K": ("vision_transformer4k", "VisionTransformer4K"), "vit4k_xs": ("vision_transformer4k", "vit4k_xs"),
    "ResNet_Baseline": ("resnet_custom", "ResNet_Baseline"), "Bottleneck_Baseline": ("resnet_custom", "Bottleneck_Baseline"),
    "resnet50_baseline": ("resnet_custom", "resnet50_baseline"),
    # HistoResNet-18 (the stub resnet_custom.resnet18_baseline still raises: DESIGN.md 15)
    "ResNet18_Baseline": ("resnet18", "ResNet18_Baseline"), "BasicBlock_Baseline": ("resnet18", "BasicBlock_Baseline"),
    "resnet18_baseline": ("resnet18", "resnet18_baseline"),
    "install": ("dropin", "install"), "build_native": ("_native", "build"),
    "FeatureWriter": ("feature_store", "FeatureWriter"), "extract_slide": ("feature_store", "extract_slide"),
    "load_bag": ("feature_store", "load_bag"), "load_coords": ("feature_store", "load_coords"),
    # DRAS-MIL attention-guided sampling inference (eval.py --sampling)
    "SamplingConfig": ("sampling", "SamplingConfig"), "dras_eval_slide": ("sampling", "dras_eval_slide"),
    "knn": ("sampling", "knn"), "update_sampling_weights": ("sampling", "update_sampling_weights"),
    "generate_sample_idxs": ("sampling", "generate_sample_idxs"), "resnet_patch_features": ("sampling", "resnet_patch_features"),
    # bootstrapped evaluation metrics (bootstrapping.py)
    "bootstrap_metrics": ("bootstrap", "bootstrap_metrics"), "bootstrap_eval_dir": ("bootstrap", "bootstrap_eval_dir"),
    # attention heat-maps (WholeSlideImage.visHeatmap)
    "heatmap_overlay": ("heatmap", "heatmap_overlay"), "render_heatmap": ("heatmap", "render_heatmap"),
    "vis_heatmap": ("heatmap", "vis_heatmap"),
    # heat-map scores on the device: percentile ranks, reference percentiles, ROI sampling, the patch-scoring loop body
    "score_counts": ("heatmap", "score_counts"), "to_percentiles": ("heatmap", "to_percentiles"),
    "score2percentile": ("heatmap", "score2percentile"), "sample_rois": ("heatmap", "sample_rois"),
    "compute_from_batches": ("heatmap", "compute_from_batches"),
    # hierarchical region attention heat-maps (create_hierarchical_heatmaps_indiv, HIPT_4K.get_region_attention_heatmaps)
    "hierarchical_heatmaps": ("hier_heatmap", "hierarchical_heatmaps"), "compose_heatmaps": ("hier_heatmap", "compose_heatmaps"),
    "region_attention_maps": ("hier_heatmap", "region_attention_maps"), "shifted_regions": ("hier_heatmap", "shifted_regions"),
    "colour_table_n": ("hier_heatmap", "colour_table_n"), "cmap_map": ("hier_heatmap", "cmap_map"),
    "create_hierarchical_heatmaps_indiv": ("hier_heatmap", "create_hierarchical_heatmaps_indiv"),
    "hierarchical_heatmaps_concat_select": ("hier_heatmap", "hierarchical_heatmaps_concat_select"),
    "create_hierarchical_heatmaps_concat_select": ("hier_heatmap", "create_hierarchical_heatmaps_concat_select"),
    # patch-level ViT-256 attention heat-maps in batches (create_patch_heatmaps_indiv, create_patch_heatmaps_concat)
    "patch_heatmaps": ("patch_heatmap", "patch_heatmaps"), "compose_patch_heatmaps": ("patch_heatmap", "compose_patch_heatmaps"),
    "patch_attention_maps": ("patch_heatmap", "patch_attention_maps"), "shifted_patches": ("patch_heatmap", "shifted_patches"),
    "create_patch_heatmaps_indiv": ("patch_heatmap", "create_patch_heatmaps_indiv"),
    "create_patch_heatmaps_concat": ("patch_heatmap", "create_patch_heatmaps_concat"),
    # patch coordinates from tissue contours (WholeSlideImage.process_contour, the contour checking functions)
    "point_polygon_test": ("tiling", "point_polygon_test"), "process_contour": ("tiling", "process_contour"),
    "process_contours": ("tiling", "process_contours"), "process_contours_like": ("tiling", "process_contours_like"),
    "pack_slide": ("tiling", "pack_slide"), "plan_contours": ("tiling", "plan_contours"),
    # Pillow's Image.resize of uint8 RGB images (the heat-maps' background, the ResNet routes' patch resize)
    "resize_u8": ("resize", "resize_u8"), "resize_table": ("resize", "resize_table"), "resize_patches": ("resize", "resize_patches"),
    # Macenko stain normalisation of uint8 RGB images (extract_features_fp.py --use_transforms macenko)
    "macenko_fit": ("macenko", "macenko_fit"), "macenko_apply": ("macenko", "macenko_apply"),
    "macenko_normalize": ("macenko", "macenko_normalize"), "MacenkoNormalizer": ("macenko", "MacenkoNormalizer"),
    "extract_slide_normalised": ("feature_store", "extract_slide_normalised"),
    # tensor-space augmentation of uint8 RGB regions (extract_features_fp.py --use_transforms all / spatial)
    "TENSOR_POLICIES": ("tensor_augment", "TENSOR_POLICIES"), "draw_tensor_params": ("tensor_augment", "draw_tensor_params"),
    "augment_tensor": ("tensor_augment", "augment_tensor"), "TensorAugment": ("tensor_augment", "TensorAugment"),
    # the tissue mask of WholeSlideImage.segmentTissue (saturation, median, threshold / Otsu, closing) and its contour filter
    "tissue_mask": ("segment", "tissue_mask"), "segment_tissue": ("segment", "segment_tissue"),
    "saturation_u8": ("segment", "saturation_u8"), "median_blur_u8": ("segment", "median_blur_u8"),
    "otsu_threshold": ("segment", "otsu_threshold"), "morph_close_u8": ("segment", "morph_close_u8"),
    "contour_area": ("segment", "contour_area"), "filter_contours": ("segment", "filter_contours"),
    # cv2.findContours(mask, RETR_CCOMP, CHAIN_APPROX_NONE) on the device: the step between the mask and the contour filter
    "trace_contours": ("segment", "trace_contours"), "find_contours": ("segment", "find_contours"),
    # WholeSlideImage.get_seg_mask: the contours filled on the device (cv2.drawContours, thickness=-1), the heat-maps' mask
    "seg_mask": ("segment", "seg_mask"), "get_seg_mask_like": ("segment", "get_seg_mask_like"),
    "scale_contours": ("segment", "scale_contours"), "scale_holes": ("segment", "scale_holes"),
}


def __getattr__(name):
    if name in _LAZY:
        import importlib
        mod, attr = _LAZY[name]
        return getattr(importlib.import_module(f"{__name__}.{mod}"), attr)
    raise AttributeError(name)
