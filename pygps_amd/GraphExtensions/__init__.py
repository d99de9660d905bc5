"""Semi-supervised learning on graphs (reference: pyGPs/GraphExtensions): helpers that turn a kernel matrix over the nodes
of a graph into the (M1, M2) pair of ``cov.Pre``, and kernels on the nodes of a graph.

    from pygps_amd.GraphExtensions import graphUtil, nodeKernels

Index work and O(n^2) arithmetic run on the host in numpy; the O(n^3) node kernels and the k-NN graph construction run on
the device (csrc/graph.hip)."""
from . import graphUtil, nodeKernels  # noqa: F401
