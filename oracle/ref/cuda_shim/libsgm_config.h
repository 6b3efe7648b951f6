// stand-in for the header libsgm's CMake configures (version numbers and the shared-library switch): a static build
#pragma once
#define LIBSGM_VERSION 0
#define LIBSGM_VERSION_MAJOR 0
#define LIBSGM_VERSION_MINOR 0
#define LIBSGM_VERSION_PATCH 0
