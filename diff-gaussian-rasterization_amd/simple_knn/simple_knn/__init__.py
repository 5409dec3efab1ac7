"""Drop-in for simple-knn's `simple_knn` package (3DGS, MonoGS, Photo-SLAM, Gaussian-SLAM, the CG-SLAM family:
`from simple_knn._C import distCUDA2`).

Put this directory's parent (`.../diff-gaussian-rasterization_amd/simple_knn`) and the package root
(`.../diff-gaussian-rasterization_amd`) on PYTHONPATH.
"""
