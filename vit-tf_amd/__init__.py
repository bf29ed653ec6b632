"""vit-tf hot path, MI355X-native: DINO ViT K-feature volumes + similarity queries through hand-written
HIP kernels (libvittf.so, C ABI in include/vittf.h).  Importing the package does not touch the GPU;
every compute entry point raises if the library or a gfx950 device is missing (no CPU fallback)."""
from . import _lib                                                  # noqa: F401
from ._lib import VittfError                                        # noqa: F401
from .weights import (ARCHS, synthetic_state_dict, load_state_dict_file, find_local_checkpoint,   # noqa: F401
                      fold_patch_embed, fold_layer_scale, interpolate_pos_embed, rope_table, dinov3_from_hf)
from .engine import HipViT                                          # noqa: F401
from .extract import (sizing, feature_volume, pooled_axis, k_slices, DeviceVolume, AXIS_DIMS)     # noqa: F401
from .similarity import sample_features3d, compute_similarities, assign_labels                    # noqa: F401
from .synthetic import synthetic_volume, ct_like_volume, shapes                                   # noqa: F401
from . import bilateral, components, distance, forest, kmeans, knn, mlp, pca, render, samplers, scores, similarity, svm, voxel_features, weights                    # noqa: F401
from .pca import (Basis, feature_gram, basis_from_gram, fit_basis, project, reduce_features,     # noqa: F401
                  save_basis, load_basis, rgb_volume)
from .kmeans import Clustering, save_clustering, load_clustering                                 # noqa: F401
from .svm import SvmModel, save_model                                                            # noqa: F401
from .forest import ForestModel                                                                  # noqa: F401
from .mlp import MlpModel                                                                        # noqa: F401
from .knn import KnnModel                                                                        # noqa: F401


def load_model(path):
    """The model of a file svm.save_model or knn.save_model wrote: a k-NN bank names itself (format = 'vittf-knn-1'); anything
    else goes to svm.load_model, as before."""
    return knn.load_model(path) if knn.is_knn_file(path) else svm.load_model(path)

__all__ = ['HipViT', 'feature_volume', 'compute_similarities', 'sample_features3d', 'assign_labels',
           'synthetic_state_dict', 'sizing', 'VittfError']
