// Forced in front of ONE of libsgm's sources, census_transform.cu (oracle/ref/Makefile: -include), after the CUDA stand-in.
// census_transform_kernel writes a feature only where the whole 9 x 7 window lies inside the image
// (census_transform.cu:76: half_kw <= x < width - half_kw, half_kh <= y < height - half_kh), and the feature image is a
// DeviceBuffer that cudaMalloc's and never clears (device_buffer.hpp:44).  The path kernels then read the features of
// EVERY pixel (left[x + y * width], right[x - d]), the 4-column / 3-row border included.  So libsgm's answer depends on
// what a fresh device allocation holds: with the stand-in's cudaMalloc filling 0x00 and then 0xFF, both census images,
// all eight path volumes and — on textured pairs — every disparity image differ between the two runs
// (tests/test_oracle_pinned_sgm.py's two-fill test, before this pin).  On a GPU a fresh allocation of a new process is
// zero pages in practice; oracle/sgm.c and the HIP kernel take the border as 0.  This header pins exactly that buffer to
// zero so that the compiled reference is a function of its inputs: the DeviceBuffer<feature_type> constructor is
// instantiated in this translation unit only (CensusTransform<T>::enqueue), and no other allocation is.  Every other
// allocation of the library keeps the fill byte.  Nothing else of the source changes.
#pragma once
#define cudaMalloc(p, bytes) cuda_shim_malloc_zero((p), (bytes))
