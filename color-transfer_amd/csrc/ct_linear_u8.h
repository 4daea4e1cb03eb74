// ct_linear_u8.h -- host-side interface of linear_u8.hip for linear.hip: ct_workspace_bytes() lives there and answers for
// CT_WS_MK_U8 with the layout that linear_u8.hip carves.
#pragma once
#include <stddef.h>

namespace ct {

// bytes of workspace ct_mk_u8 needs for `batch` pairs (the frame size does not enter)
size_t ws_bytes_mk_u8(int batch);

}  // namespace ct
