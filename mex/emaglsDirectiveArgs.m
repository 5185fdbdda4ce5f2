function [rot, coef] = emaglsDirectiveArgs(sourceOrientation, directivity, Q, P)
% 'sourceOrientation' and 'directivity' of getArrayIrs / getArrayRoomIrs as the gateway takes them (DESIGN.md section 15).
%   directivity        [Q x Kd x P], real or complex; [Q x Kd] or a vector [Kd] is repeated over bins and sources; Kd = (Nd + 1)^2
%   sourceOrientation  [3 x 3 x Q] rotation matrices whose columns are each source's front, left and up axes in room axes, or
%                      [Q x 2] = (azimuth, zenith) of the front axis with zero roll, R = Rz(azi) * Ry(zen - pi/2); []: the room's axes
%   rot                [Q x 9], row q = R_q row by row, or []
%   coef               [Q*Kd x P], row (q - 1) * Kd + i = c_{q,i}
c = directivity;
if isvector(c); c = reshape(c, 1, []); end      % (a vector is [Kd], also when it has Q elements)
if size(c, 1) == 1; c = repmat(c, [Q 1 1]); end
if size(c, 3) == 1; c = repmat(c, [1 1 P]); end
if size(c, 1) ~= Q || size(c, 3) ~= P
    error('eMagLS:arg', 'directivity must be [Q x Kd x P] (Q = %d sources, P = nfft/2 + 1 = %d bins), [Q x Kd] or [Kd]', Q, P);
end
Kd = size(c, 2);
if (round(sqrt(Kd)))^2 ~= Kd; error('eMagLS:arg', 'directivity holds %d coefficients per source and bin, which is not a square (Nd + 1)^2', Kd); end
coef = reshape(permute(c, [2 1 3]), Q * Kd, P);
rot = [];
o = double(sourceOrientation);
if ~isempty(o)
    if ismatrix(o) && isequal(size(o), [Q 2])
        R = zeros(3, 3, Q);
        for q = 1:Q
            a = o(q, 1); b = o(q, 2) - pi / 2;
            R(:, :, q) = [cos(a) -sin(a) 0; sin(a) cos(a) 0; 0 0 1] * [cos(b) 0 sin(b); 0 1 0; -sin(b) 0 cos(b)];
        end
        o = R;
    end
    if size(o, 1) ~= 3 || size(o, 2) ~= 3 || size(o, 3) ~= Q
        error('eMagLS:arg', 'sourceOrientation must be [3 x 3 x Q] rotation matrices or [Q x 2] (azimuth, zenith) of the front axis');
    end
    rot = reshape(permute(o, [2 1 3]), 9, Q).';
end
end
