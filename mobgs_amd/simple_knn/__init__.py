"""Drop-in for the reference's `simple_knn` package (a CUDA-only extension upstream): `from simple_knn._C import
distCUDA2` becomes `from mobgs_amd.simple_knn._C import distCUDA2`."""
from ._C import distCUDA2  # noqa: F401
