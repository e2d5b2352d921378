#pragma once
#include "host_util.h"
#include "../../include/etude_hip.h"
