"""The reference's utils/flow_viz.py entries the models call, on the device (ct_hip.flow_to_image, csrc/views.hip): the Middlebury
colour code of a flow field.  Device tensors in, device uint8 tensors out; no CPU path, and the argument is not modified (the
reference zeroes the unknown pixels of its numpy argument in place)."""
import ct_hip


def flow_to_image(flow):
    """flow_viz.py:229-264: one [H,W,2] flow -> [H,W,3] uint8"""
    if flow.dim() != 3 or flow.shape[2] != 2:
        raise ValueError("flow_to_image needs one [H,W,2] flow")
    return ct_hip.flow_to_image(flow.permute(2, 0, 1).unsqueeze(0).float().contiguous())[0]


def flow_tensor_to_image(flow):
    """flow_viz.py:272-279: one [2,H,W] flow -> [3,H,W] uint8 (a view of the [H,W,3] image), what GMFlow's pred_flow_viz returns
    per sample: flow_tensor_to_image(result["flow"][i])"""
    if flow.dim() != 3 or flow.shape[0] != 2:
        raise ValueError("flow_tensor_to_image needs one [2,H,W] flow")
    return ct_hip.flow_to_image(flow.unsqueeze(0).float().contiguous())[0].permute(2, 0, 1)
