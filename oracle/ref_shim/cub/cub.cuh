// cub::DeviceScan / cub::DeviceRadixSort -> hipcub (rocPRIM back end)
#pragma once
#include <hipcub/hipcub.hpp>
namespace cub = hipcub;
