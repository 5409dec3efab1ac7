// included by the reference, nothing of it is used
#pragma once
#include "../cooperative_groups.h"
