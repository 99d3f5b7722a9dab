// rt_usd_internal.h — shared among the USD readers (rt_usd*.cpp); their users include rt_usd.h only.
#pragma once
#include "rt_file.h"   // read_file
#include "rt_usd.h"

namespace rt {
namespace usd {

inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }
float half_to_float(uint16_t h);
int element_size(double d);   // primvar elementSize from a file number
// one layer by content: "PXR-USDC" crate or "#usda" text
bool parse_layer(const uint8_t* data, size_t n, Stage& st, std::string& err);

}  // namespace usd
}  // namespace rt
