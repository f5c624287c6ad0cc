/* TEST INFRASTRUCTURE ONLY: forwards to the host shim of the CUDA surface. */
#pragma once
#include "kfx_ref_shim.h"
