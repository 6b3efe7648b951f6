// stand-in (see cuda_runtime.h); CUDA_VERSION comes from the build line
#pragma once
#include "cuda_runtime.h"
