"""Evaluation metrics: the two that consume the exact kNN kernel -- mirror of ``torchdr/eval`` (reference
``eval/neighborhood_preservation.py:15-200`` and ``eval/knn_labels.py:17-190``) and the exact
silhouette (``eval/silhouette.py``) on its own matrix-free kernel, and ``kmeans_ari`` (``eval/kmeans.py``) on the Lloyd
k-means kernels."""

from .neighborhood_preservation import neighborhood_preservation  # noqa: F401
from .knn_labels import knn_label_accuracy  # noqa: F401
from .silhouette import silhouette_samples, silhouette_score, admissible_LIST_METRICS  # noqa: F401
from .kmeans import kmeans_ari  # noqa: F401
