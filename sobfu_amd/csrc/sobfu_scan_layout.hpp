// The block sizes of the shared int scan (sobfu_scan.hpp) without its kernels: a unit that only reads a layout made with the scan (the
// triangle grid's readers, sobfu_mesh.hpp) needs kChunk and should not compile kernels it never launches.
#pragma once
namespace sobfu_hip {
namespace {
constexpr int kBlock = 256, kItems = 8, kChunk = kBlock * kItems;  // cells per workgroup
}
}  // namespace sobfu_hip
