"""`simple_knn._C`: distCUDA2(points [N,3]) -> [N] mean squared distance to the three nearest neighbours
(/root/reference/scene/gaussian_model.py:10, :420, :514), computed by csrc/knn.hip."""
from ..scene_init import knn3_mean_dist2


def distCUDA2(points):
    return knn3_mean_dist2(points)
