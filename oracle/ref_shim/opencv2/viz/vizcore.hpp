/* TEST INFRASTRUCTURE ONLY: nothing of cv::viz is used by the kernels built against this shim. */
#pragma once
