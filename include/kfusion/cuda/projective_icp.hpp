// Forwarding header: the reference include path <kfusion/cuda/projective_icp.hpp> resolves to the MI355X shells.
#pragma once
#include <sobfu_amd/sobfu.hpp>
