"""Graph extensions (reference: pyGPs/GraphExtensions): helpers that turn a kernel matrix over the nodes of a graph, or over
whole graphs, into the (M1, M2) pair of ``cov.Pre``; kernels on the nodes of a graph; propagation kernels between graphs.

    from pygps_amd.GraphExtensions import graphUtil, nodeKernels, graphKernels

Index work and O(n^2) arithmetic run on the host in numpy; the O(n^3) node kernels and the k-NN graph construction
(csrc/graph.hip) and the propagation kernel's iterations (csrc/propagate.hip) run on the device."""
from . import graphUtil, nodeKernels, graphKernels  # noqa: F401
